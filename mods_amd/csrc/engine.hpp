// engine.hpp -- internal types of libmodsx (device job descriptors, context, host helpers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/modsx.h"
#include "kmath.hpp"
#include "fginn_walk.hpp"

namespace mx {

// ---- device job descriptors (passed by value in kernel arguments) ----------------------
#ifndef MODSX_MAXB
#define MODSX_MAXB 32
#endif
constexpr int MAXB = MODSX_MAXB;   // images (views) per batched launch set: 8 / 16 / 32 measured 150 / 157 / 159 pairs/s at 31 views
constexpr int PAIR_GROUP = 4;      // identity-view pairs per launch set of modsx_match_pairs (8 images; 16 measured slower)
constexpr int NMS_MAXJ = 1024; // (image, octave, level) jobs per NMS launch (flushed when full)
constexpr int MAX_TAPS = 17;   // pyramid kernels: ksize <= 17

struct BlurJob {
  const float *src;
  float *blur;   // may alias nothing; nullptr for k_hessian
  float *resp;   // nullptr = no response
  int rows, cols;
  float norm;    // sigma^2 passed to HessianResponse
  int pad;
};
struct BlurBatch {
  int n;                 // ksize
  float k[MAX_TAPS];
  BlurJob j[MAXB];
  int nj;                // jobs in use; tile0[i] = first tile of job i in the flat tile list of the launch (filled by the launcher)
  int tile0[MAXB + 1];
};
struct ResizeJob {
  const float *src;
  float *dst;
  float *resp;   // not null: the Hessian response of the resized level is written too (norm = its sigma^2)
  int srows, scols, drows, dcols;
  float norm;
  int pad;
};
struct ResizeBatch { ResizeJob j[MAXB]; int nj; int tile0[MAXB + 1]; };
struct NmsJob {
  const float *low, *cur, *high, *blur;
  int rows, cols, img, octave, level, pad;
};
struct NmsBatch {   // thresholds of one scan; the (image, octave, level) jobs and their tile prefix live in device memory
  float posTh, negTh, finalTh;
  int border;
  double edgeScoreThreshold;
  int detType, pad;      // getPointType (pyramid.cpp:66-130): Hessian dark / bright / saddle, DoG 10 / 11, Harris 30 / 31
};
struct Candidate {
  int img, octave, level, type;
  int r0, c0, r, c;
  float b0, b1, b2, val;
};

// Baumberg: one wave per scale-space keypoint
// external form (launch_baumberg_external, DetectAffineShape on a caller's regions): blur = the view image, x, y = the position in
// it, s = the RATIO the window steps by (formed by the host in f64), pixelDistance is not read
struct AffJob {
  const float *blur;  // prevBlur level
  int rows, cols;
  float x, y, s, pixelDistance;
};
struct AffOut { float u11, u12, u21, u22; int ok; int iters; };

// orientation: one wave per region
struct OriJob {
  int img;
  float x, y, a11, a12, a21, a22;  // A * curr_sc, f32 (synth-detection.cpp:892-898)
};
// orientation results: (1 + maxA) 32-bit words per region -- the angle count, then the angles; maxA = min(maxAngles, 18), the
// most strict local maxima a 36-bin circular histogram can have (so "all peaks", maxAngles = -1, loses none)
constexpr int ORI_MAX_PEAKS = 18;

// describe
struct DescJob {
  int img;
  int P;              // patchImageSize (+2 when smoothed), 0 = direct mode
  int ksize;          // blur kernel size for 1.5*imageToPatchScale
  int tapOfs;         // offset into the tap table
  float x, y, a11, a12, a21, a22;   // direct mode: A * imageToPatchScale
  float i2p;          // imageToPatchScale
  int NC;             // number of window columns (= rows) the 41x41 resampling reads (<= 82)
  int needOfs;        // offset into the int table: NC needed indices, then 41 x {idx of x0, idx of x0+1, valid}
  int coordOfs;       // offset into the float table: 41 sample coordinates WX_i (= WY_j)
  int touch;          // interpolate()'s border branch for the 41x41 resampling
  int outIdx;         // index of the region in its image's descriptor buffers
  int rows0;          // window rows per workgroup of the LDS row filter, 0 = this job goes through k_patch_blur
  int ro1;            // needed rows per workgroup of the LDS column filter, 0 = k_patch_blur, -1 = the fused sampling kernel
                      // filters the columns too (small window: whole row tile + row-filtered block fit its LDS)
  unsigned long long scratchOfs;    // float offset of this region's P x P window (arena A); for windows that take the fused
                                    // sample + row-filter kernel: float2 offset of its P row starts
  unsigned long long rowOfs;        // float offset of its P x NC row-filtered block (arena B)
  unsigned long long gridOfs;       // float offset of its NC x NC blurred grid (arena C)
};
struct BlurTile {     // one workgroup of the LDS blur kernels
  unsigned long long srcOfs, dstOfs;   // float offsets: first input row / first output of the tile
  int P, NC, n, tapOfs, needOfs;
  int job, pad;                        // index of the tile's DescJob (the fused sample + row-filter kernel reads its affine frame)
  int first, count, lo, span, magic;  // rows pass: window rows [first, first+count); columns pass: needed rows, parked source rows [lo, lo+span); magic = ceil(2^20 / ceil(NC / 2))
};
struct ImgRef { const float *d; int rows, cols, pad; };
// per image of the batch: [n][128] f32 and u8 descriptors of the step's first descriptor class, u8 of up to three more
struct DescOut { float *f[MAXB]; uint8_t *u8[MAXB]; uint8_t *u8x[3][MAXB]; };

// view synthesis
struct WarpJob {
  const float *src;
  float *dst;
  int srows, scols, drows, dcols;
  double M[6];   // inverse map (dst -> src), already inverted on the host in f64
  float cval;
  int pad;
};

// one non-identity view of a batched synthesis (kernels_views.hip): src -R-> rot -blur (through tmp)-> rot -W-> dst;
// a view of the one-launch form (fused == 2) goes src -> dst and has no rot / tmp
struct ViewJob {
  const float *src;
  float *rot, *tmp, *dst;
  int srows, scols, rrows, rcols, drows, dcols;
  int kx, ky, tapOfs, doBlur;
  int tileA, tileB;   // first 64 x 4 tile of this view in the rotated-image / output-image tile lists
  int tileF, fused;   // fused rotate + blur: first VF_TW x VF_TH tile of this view (views with a blur whose halo fits)
  int tileG, pad;     // rotate + blur + tilt in one launch (fused == 2: W is diagonal as well): first VF_TW x VF_TH tile of the ROTATED image
  // fused == 2: the views that share this view's rotation (same src, sizes and R, bit for bit) lie next to each other in the job
  // table and share tileG: one workgroup rotates a tile once for all of them
  int grpFirst, grpCount;   // table index of the group's first view, views in the group (1 .. VIEW_GROUP_CAP)
  int grpRx, grpRy;         // largest kx >> 1 / ky >> 1 of the group: the halo of the shared rotated tile
  double R[6], W[6];  // inverse maps of the two cv::warpAffine calls (f64, inverted on the host)
  double invW[2];     // 1 / W[0], 1 / W[4]: where a fused tile starts looking for its first output column / row (a hint, never the answer)
};

// matching
struct MatchRow {     // per-query result of the device matcher
  int t0, t1, nless, nbad;
  int tj;             // (tj, dj) is one 8-byte word (dj the high half): k_match_resolve takes the minimum of (distance, train)
  float dj;           // over the splits with a 64-bit atomic -- positive floats order like their bits
  float d0, d1;
};
static_assert(sizeof(MatchRow) == 32, "match rows are 32 bytes");

// ---- host side ---------------------------------------------------------------------------
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  bool ensure(size_t bytes);
  void release();
};
struct PinBuf {
  void *p = nullptr;
  size_t cap = 0;
  bool ensure(size_t bytes);
  void release();
};

struct Octave {
  int rows, cols;
  float pixelDistance;
  float *blur[8];
  float *resp[8];
};
struct Pyramid {
  int nOct = 0;
  Octave oct[24];
  DevBuf store;
};

void set_error(const std::string &s);
// How many contexts are inside a call that keeps the device busy (a pair, a view set, a matching problem).  One: the call has the GPU
// to itself and may launch shapes that take whole CUs (k_match_sweep1's fat workgroups: -4 % alone); more: its launches share the
// CUs with the other contexts' and stay good neighbours (the fat shape waits for a drained CU there: -0.4 % pairs/s under 16 streams).
bool gpu_shared();
struct CtxBusy { modsx_ctx *c; explicit CtxBusy(modsx_ctx *c); ~CtxBusy(); CtxBusy(const CtxBusy &) = delete; CtxBusy &operator=(const CtxBusy &) = delete; };
// stage boundaries without the runtime's copy / wait calls (engine.hip): a kernel copies between device and PINNED host memory,
// a one-lane kernel writes a sequence number into the context's pinned flag word, the host thread naps until it sees it
hipError_t ctx_copy(modsx_ctx *c, void *dst, const void *src, size_t bytes, hipMemcpyKind kind);
hipError_t ctx_sync(modsx_ctx *c);
unsigned ctx_mark(modsx_ctx *c);
bool ctx_mark_reached(modsx_ctx *c, unsigned seq);
hipError_t ctx_wait_mark(modsx_ctx *c, unsigned seq);
bool host_wait_runtime();
int host_cpus_per_rank();      // mser.cpp: CPUs this process may use (cgroup allowance / local ranks)
#define MX_HIP(expr)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      mx::set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                       \
      return MODSX_ERR_DEVICE;                                                                \
    }                                                                                         \
  } while (0)

// tables.cpp (host precomputation, reference semantics)
std::vector<float> gaussian_kernel(int n, double sigma);
int blur_ksize(float sigma);
void gauss_mask(float *mask, int size);
void circular_gauss_mask(float *mask, int size, float sigma);
const double *atan_lut_host();
inline bool check_borders_host(int w, int h, float ofsx, float ofsy, float a11, float a12, float a21, float a22, int rw, int rh) {
  return check_borders(w, h, ofsx, ofsy, a11, a12, a21, a22, rw, rh);     // kmath.hpp (host build of the kernels' expression)
}
bool invert3(const double *S, double *t);
void rectify(double &a11, double &a12, double &a21, double &a22);

// kernel launchers
// the tile height of a k_blur_hess launch over n planes and its tile count (host only): 32-row tiles when they fill two rounds of
// workgroups, 16-row tiles below that (kernels_pyramid.hip)
struct BlurGeo { int th, tiles; };
BlurGeo blur_geometry(const int *rows, const int *cols, int n);
// what launch_blur_hess launched: th = 0 when the batch held no pixel, R = the instantiated half width (1..8)
struct BlurLaunch { int th, tiles, R; };
BlurLaunch launch_blur_hess(hipStream_t s, const BlurBatch &b, int nj, int maxRows, int maxCols);
bool launch_hessian(hipStream_t s, const BlurBatch &b, int nj, int maxRows, int maxCols);        // false: nothing to launch
bool launch_resize_half(hipStream_t s, const ResizeBatch &b, int nj, int maxRows, int maxCols);
void launch_nms(hipStream_t s, const NmsBatch &b, const NmsJob *jobs, const int *tilePrefix, const int *tileJob, int nj,
                int nTiles, int4 *queue, unsigned *qcount, unsigned qcap, Candidate *out, unsigned *counter, unsigned cap,
                const int *octFirst = nullptr, int levelsPerOctave = 0);
size_t cand_sort_temp_bytes(unsigned nsort);
int launch_cand_order(hipStream_t s, const Candidate *cand, const unsigned *counter, unsigned nsort, unsigned long long *keys,
                      unsigned long long *keys2, unsigned *idx, unsigned *idx2, void *temp, size_t tempBytes, unsigned long long *tabKey,
                      unsigned *tabRank, unsigned tabSize, unsigned *slotOf, Candidate *out, unsigned *outCount);
constexpr int NMS_QUEUES = 64;      // sub-queues of the NMS extremum queue; counter k lives at counter[32 * (k + 1)]
constexpr int NMS_TILE_ROWS = 16;   // rows of a 64-column NMS tile (kernels_pyramid.hip: NMS_ROWS)
void launch_gray(hipStream_t s, const void *src, float *dst, size_t n, int channels, int dtype);
// kernel 0 = k_baumberg_stream on static chunks, 1 = k_baumberg<19>, 2 = k_baumberg<0>, 3 = k_baumberg_stream fed from the launch-wide
// queue (-1: refused); kernels 0..2: keypoints per wavefront, wavefronts with work, workgroups; kernel 3: wavefronts per range, ranges,
// workgroups
struct BaumGeo { int kernel, chunk, nchunks, grid; };
BaumGeo baumberg_geometry(int n, int W, int variant, int chunk, int resident = 0);   // kernels_affine.hip (host only)
int baumberg_resident_waves();                                     // wavefronts of the queue form the current device holds at once
int baumberg_production_variant(int W);                            // the variant detect_keypoints_batch launches at window W
// the queue form's counters: one per range of the job list, 128 bytes apart.  They live behind the NMS counters in the context's
// counter block, which scan_extrema zeroes once per launch set and nothing touches between that fill and the Baumberg launch
constexpr int BAUM_RANGES = 8, BAUM_COUNTER_STRIDE = 32, BAUM_QUEUE_BYTES = BAUM_RANGES * BAUM_COUNTER_STRIDE * 4;
MX_HD int baum_range_start(int n, int r) { return (int)(((long long)n * r) / BAUM_RANGES); }   // range r = keypoints start(r) .. start(r + 1)
bool launch_baumberg(hipStream_t s, const AffJob *jobs, AffOut *out, int n, const float *mask, int W, int maxIter,
                     float convTh, float affInitialSigma, int variant, int chunk, int resident, unsigned *queue, bool queueClean);
bool launch_baumberg_external(hipStream_t s, const AffJob *jobs, AffOut *out, int n, const float *mask, int W, int maxIter,
                              float convTh, int variant, int chunk, int resident, unsigned *queue, bool queueClean);
constexpr int ATAN_CASES = 2048 + 64;   // 8 x 256 (sign / octant bits, table index) values of atan2LUTff's angle + the special case (entry 2048), padded
constexpr int ORI_NV = 1344;   // entries of the orientation kernel's voting-pixel list (1245 under the mask, padded to 64 lanes x 21)
constexpr int ORI_PSP = 44;    // row stride of the orientation kernel's padded 41 x 41 patch: what the voting list indexes
// fewer regions than two rounds of wavefronts over the chip: k_orientation reads the bin table from a copy in LDS, otherwise
// where it lies in global memory (kernels_orient.hip)
constexpr int ORI_LDS_TABLE_BELOW = 2 * 256 * 16;
inline bool orientation_lds_table(int n) { return n < ORI_LDS_TABLE_BELOW; }
void launch_orientation(hipStream_t s, const OriJob *jobs, float *out, int n, const ImgRef *imgs,
                        const unsigned short *maskIdx, const float *maskW,
                        const unsigned char *binTab, int doHalf, double th, int maxAngles);
// The host-built tables of k_orientation (engine.hip): what upload_tables copies to the device and modsx_orientation_tables shows.
struct OriTables {
  std::vector<unsigned char> binTab;                 // ATAN_CASES: histogram bin of atan2LUT case code * 256 + idx, [2048] the special case
  std::vector<unsigned short> idxRaster, idxLanes;   // ORI_NV: r * ORI_PSP + q of the voting pixels in raster order / as uploaded
  std::vector<float> wRaster, wLanes;                // ORI_NV: their mask values (0 in the padding)
  int nReal = 0;                                     // voting pixels before the padding
};
int orientation_tables_host(OriTables &t);           // MODSX_OK, or MODSX_ERR_ARG with the error text set
void launch_trunc_u8(hipStream_t s, const float *src, uint8_t *dst, size_t n);
size_t mser_sort_blocks(const int *rows, int n);
void launch_mser_sort(hipStream_t s, const uint8_t *const *u8, const int *rows, const int *cols, const size_t *ordOfs, int n, int *blockHist,
                      int *start, int *order);
void launch_expand_blur_tiles(hipStream_t s, const DescJob *jobs, const int *prefixRows, const int *prefixCols, int nJobs,
                              const int *needTab, BlurTile *tilesRows, BlurTile *tilesCols, float2 *rowStarts);
void launch_sample_rows(hipStream_t s, const DescJob *jobs, const BlurTile *tiles, int nTiles, const ImgRef *imgs, const float *taps,
                        const int *needTab, float *dst, const float2 *rowStarts, float *dstGrid);
void launch_blur_cols(hipStream_t s, const BlurTile *tiles, int nTiles, const float *taps, const int *needTab, const float *src,
                      float *dst);
void launch_expand_tiles(hipStream_t s, const int *prefix, int nJobs, int *tileJob);
void launch_patch_sample(hipStream_t s, const DescJob *jobs, const int *tilePrefix, const int *tileJob, int nTiles,
                         const ImgRef *imgs, float *scratch);
void launch_patch_blur(hipStream_t s, const DescJob *jobs, const int *tilePrefix, const int *tileJob, int nTiles,
                       const float *taps, const int *needTab, const float *src, float *dst, int pass);
// redo: null for today's kernel; else the launch set's redo list (a zero count word, 12 spare bytes, one entry per two jobs),
// with which a launch whose jobs are all grid-branch ones takes the slim form and its redo launch.  orderedCnt: two words (the
// ordered workgroups, the redo workgroups).  -> 1 when the slim form was launched, else 0
int launch_describe(hipStream_t s, const DescJob *jobs, int n, const ImgRef *imgs, const float *grid,
                    const int *needTab, const float *coordTab,
                    const float *mask, const unsigned short *maskIdx, int nmask, const float *oTab, const int *bins,
                    const double *wts, int photoNorm, int descTypes, int nOut, double maxBin, const DescOut &outs,
                    unsigned *orderedCnt, unsigned *redo);
void launch_warp_affine(hipStream_t s, const WarpJob &jb);
void launch_blur_pass(hipStream_t s, const float *src, float *dst, int rows, int cols, const float *taps, int n, int pass, int border = 0);
void launch_sub(hipStream_t s, const float *a, const float *b, float *o, size_t n);
void launch_grad_products(hipStream_t s, const float *img, int rows, int cols, float *xx, float *yy, float *xy);
void launch_harris_combine(hipStream_t s, const float *bxx, const float *byy, const float *bxy, float sigmasq, float *o, size_t n);
void launch_views_warp(hipStream_t s, const ViewJob *jobs, int n, int tiles, int stage);
void launch_views_blur(hipStream_t s, const ViewJob *jobs, int n, int tiles, const float *taps, int pass);
constexpr int VF_TW = 128, VF_TH = 16, VF_RX = 32, VF_RY = 2;   // tile of the fused rotate + blur kernel and the largest halo it takes
constexpr int VIEW_GROUP_CAP = 8;   // most views that share one rotated tile of k_views_fused (the shipped ladders need 4)
void launch_views_rotblur(hipStream_t s, const ViewJob *jobs, int n, int tiles, const float *taps, int maxRx, int maxRy);
void launch_views_fused(hipStream_t s, const ViewJob *jobs, int n, int tiles, const float *taps, int maxRx, int maxRy);
size_t match_workspace_bytes(int n1, int n2);
void launch_match(hipStream_t s, const uint8_t *d1, int n1, const uint8_t *d2, int n2, const double *pos2,
                  double sqminratio, double contrDistSq, int nn, MatchRow *rows, void *workspace);
// Shapes of the fused sampling + row-filter kernel (kernels_describe.hip k_sample_rows_lds; describe_plan.cpp sizes the tiles with the
// same numbers): LDS floats of the sampled row tile, block rows of a fully fused small window, whether a wave's coordinate
// park is 2 x 64 x 5 words (1) or 2 x 64 x 9 (0; describe_lanes.hpp fills 320 of them), and the workgroups per CU the kernel is built for
// The kernel's time follows its residency far more than its tile shapes: with 4 workgroups per CU (20 KB tile + 20 KB of
// coordinates / fused block) it took 1.9 ms per 31-view pair on one stream, padded to 3 per CU 3.4 ms, and at 6 / 7 / 8 per CU
// 1.33 / 1.18 / 1.13 ms (175 -> 179 / 179.5 / 180.5 pairs/s), although fewer windows are then small enough for the fused
// column pass (the separate column filter grows from 0.69 to 0.86 ms).
#ifndef MODSX_SR_WIN
#define MODSX_SR_WIN 2400
#define MODSX_FC_ROWS 40
#define MODSX_SR_HALF 1
#define MODSX_SR_WGS 8
#endif
// LDS floats of a column-filter workgroup (kernels_describe.hip k_blur_cols_lds; describe_plan.cpp sizes the tiles with the same number)
#ifndef MODSX_BLUR_LDS_C
#define MODSX_BLUR_LDS_C 9984
#endif
constexpr int MATCH_NN_MAX = 256;   // largest `nn` of the FGINN walk (matching.hpp:268-269: 50): the event kernel lists fewer than nn groups per query
constexpr int MATCH_MAXB = 4;   // independent matching problems per launch set (blockIdx.z)
void launch_match_batch(hipStream_t s, int nb, const uint8_t *const *d1, const int *n1, const uint8_t *const *d2, const int *n2,
                        const double *const *pos2, double sqminratio, double contrDistSq, int nn, MatchRow *const *rows,
                        void *const *workspace, hipEvent_t *evSweep1 = nullptr,    // evSweep1: two events recorded around sweep 1
                        const void *const *trainPack = nullptr);                   // trainPack[i]: problem i's trains were packed there
// a train set packed once (the train side of a workspace, sized by n2 alone) and used as the train side of many problems
size_t match_train_pack_bytes(int n2);
void launch_match_pack_trains(hipStream_t s, const uint8_t *d2, int n2, const double *pos2, void *pack);
void last_match_geometry(int *qs, int *fat, int *S, int *tilesPerSplit, int *ntilesUB);   // of problem 0 of the process's last launch
// A descriptor database resident in HBM (kernels_dbnn.hip): the rows packed once into the matcher's operand form.  Read-only
// after creation, so every context of its device may use it at the same time.
struct DbGeo { int TEp, TOp; };     // tiles of the even / odd parity class (multiples of 4)
struct DbSet {
  DevBuf store;                     // tiles, then the row constants
  const unsigned char *tiles = nullptr;
  const int *hrow = nullptr;
  DbGeo geo = {0, 0};
  long rows = 0;
  int dev = 0;
};
DbGeo db_geo(long n, long nOdd);
size_t db_tiles_bytes(const DbGeo &g);
size_t db_hrow_bytes(const DbGeo &g);
int db_pack_blocks(long n);         // workgroups of k_db_pack (256 rows each): the host hands it one pair of slot bases per workgroup
void launch_db_pack(hipStream_t s, const uint8_t *raw, long n, const int2 *base, long nOdd, const DbGeo &geo, unsigned char *tiles,
                    int *hrow);
void launch_db_select(hipStream_t s, int nb, const MatchRow *const *rows, const int *n1, int nn, bool allPoints, int *const *sel, int *cnt,
                      int *const *dmin);
void launch_dbnn_min(hipStream_t s, int nb, const uint8_t *const *d1, const int *n1, int *const *sel, int *cnt, int *const *dmin,
                     const DbSet &db);
// The split rule of the exact searches (Hamming, f32 and byte-row FGINN, single and grouped): a train axis of ntiles >= 1 whole tiles
// under gx blocks of 256 queries is cut into S splits of tilesPerSplit tiles.  splits = 0: production, about 2048 workgroups (eight
// per CU; four rounds at the two that the widest f32 kernels hold at a time, so that the last round's tail stays short); splits > 0:
// that many.  At most one split per tile, and no empty split.
struct SplitCut { int tilesPerSplit, S; };
inline SplitCut split_rule(int ntiles, int gx, int splits) {
  int S = splits > 0 ? splits : (2048 + gx - 1) / gx;
  S = std::max(1, std::min(S, ntiles));
  SplitCut c;
  c.tilesPerSplit = (ntiles + S - 1) / S;
  c.S = (ntiles + c.tilesPerSplit - 1) / c.tilesPerSplit;
  return c;
}
// The Hamming 2-NN search of MatchFLANNDistance (kernels_hamming.hip).  W = ceil(nbytes / 4) dwords per row, WK the kernel width
// it rounds up to; tile = trains per LDS tile; the train axis is cut into S splits of tilesPerSplit tiles; gx x S workgroups.
struct HammingGeo { int W, WK, tile, ntiles, tilesPerSplit, S, gx; };
HammingGeo hamming_geometry(int n1, int n2, int W, int splits);   // splits = 0: production; > 0: forced (at most one per tile)
size_t hamming_workspace_bytes(const HammingGeo &g, int n1);
void launch_hamming(hipStream_t s, const HammingGeo &g, const uint8_t *d1, int n1, const uint8_t *d2, int n2, int nbytes, void *work,
                    int *nn2, hipEvent_t *ev = nullptr);             // ev: three events, around the packing and the search launches
// The grouped form: np <= MATCH_MAXB problems share one stored query side; problem p has its own stored trains (rows of WK dwords,
// zero rows up to a multiple of 1024 rows: whole tiles at every WK).  This is the whole table of the launch set, passed to the
// kernels by value.  Problem p owns the splits [first[p], first[p + 1]) of tps[p] whole tiles each; entries of first behind np
// hold the total, so that no workgroup selects an unused problem.
struct HamGroup {
  const uint32_t *trains[MATCH_MAXB];
  int n2[MATCH_MAXB], ntiles[MATCH_MAXB], tps[MATCH_MAXB], S[MATCH_MAXB];
  int first[MATCH_MAXB + 1];
  int np, gx, WK, tile;
};
int hamming_kernel_width(int W);
// n2[0..G): every problem's trains; problems with n2 == 0 are left out (prob[k] = the caller's index of table problem k).  Every
// problem is cut as hamming_geometry(n1, n2, W, 0) cuts it alone: its S and tps, whatever G is.  Returns the splits in all.
int hamming_group_geometry(int n1, const int *n2, int G, int W, HamGroup &g, int *prob);
// part: [first[np]][n1][2] keys; nn2: [np][n1][4] ints
void launch_hamming_group(hipStream_t s, const HamGroup &g, const uint32_t *queries, int n1, unsigned long long *part, int *nn2);
// dst: n rows of WK dwords at their place in a stored class, from dense [n][nbytes] u8 rows of any alignment
void launch_hamming_pack_rows(hipStream_t s, const uint8_t *src, int n, int nbytes, int WK, uint32_t *dst);
// FGINN matching of f32 rows of any width (kernels_fginn32.hip).  DK = the kernel width dim rounds up to; tile = trains per LDS
// tile; the train axis is cut into S splits of tilesPerSplit tiles; gx x S workgroups of k_f32_topk.
struct Fginn32Geo { int dim, DK, tile, ntiles, tilesPerSplit, S, gx; };
// F32Open / F32Closed, an undecided query on its way to k_f32_resolve and what comes back: fginn_walk.hpp, with the host's walk
struct Fginn32Work { float *queries, *trains; unsigned long long *keys; F32Open *open; F32Closed *closed; };
Fginn32Geo fginn32_geometry(int n1, int n2, int dim, int splits);   // splits = 0: production; > 0: forced (at most one per tile)
Fginn32Geo fginn32_geometry_rows(int n1, int n2, int dim, int DK, int tile, int splits);
size_t fginn32_workspace_bytes(const Fginn32Geo &g, int n1);
Fginn32Work fginn32_work(const Fginn32Geo &g, int n1, void *work);
void launch_fginn32_topk(hipStream_t s, const Fginn32Geo &g, const float *d1, int n1, const float *d2, int n2, void *work,
                         void *flagAndTop4, hipEvent_t *ev = nullptr, int dist = MODSX_DIST_L2);
void launch_fginn32_resolve(hipStream_t s, const Fginn32Geo &g, int n1, int nu, int n2, const double *pos, double contrDistSq, void *work,
                            int dist = MODSX_DIST_L2);
void launch_fginn32_merge(hipStream_t s, const Fginn32Geo &g, const unsigned long long *keys, int n1, unsigned long long *top4);
// The same search under L1 on rows of 128 bytes (kernels_fginn_l1.hip): the geometry, workspace layout, keys and records of the f32
// search at a row of DK = 32 dwords and 128 trains per tile (fginn32_workspace_bytes / fginn32_work serve both).  d1 / d2: dense
// [n][128] u8 rows in HBM of any alignment; flagAndTop4 as above (the flag word stays 0: every byte is a valid value)
Fginn32Geo fginn_l1_geometry(int n1, int n2, int splits);
void launch_fginn_l1_topk(hipStream_t s, const Fginn32Geo &g, const uint8_t *d1, int n1, const uint8_t *d2, int n2, void *work,
                          void *flagAndTop4, hipEvent_t *ev = nullptr);
void launch_fginn_l1_resolve(hipStream_t s, const Fginn32Geo &g, int n1, int nu, int n2, const double *pos, double contrDistSq, void *work);
// The grouped form: np <= MATCH_MAXB problems share one stored query side (rows of DK floats, padded to whole workgroups); problem p
// has its own stored trains (zero rows up to a multiple of 256) and positions.  This is the whole table of the launch set, passed
// to the kernels by value.  Train axis: problem p owns the splits [first[p], first[p + 1]) of tps[p] whole tiles each.  Resolve:
// problem p owns the open entries [ubeg[p], uend[p]) and the workgroups [rfirst[p], rfirst[p + 1]) = its blocks of 256 entries x
// its splits.  Entries of first / rfirst behind np hold the total, so that no workgroup selects an unused problem.
struct F32Group {
  const float *trains[MATCH_MAXB];
  const double *pos[MATCH_MAXB];
  int n2[MATCH_MAXB], ntiles[MATCH_MAXB], tps[MATCH_MAXB], S[MATCH_MAXB];
  int first[MATCH_MAXB + 1];
  int ubeg[MATCH_MAXB], uend[MATCH_MAXB], rfirst[MATCH_MAXB + 1];
  int np, gx, DK, tile;
};
// n2[0..G): every problem's trains; problems with n2 == 0 are left out (prob[k] = the caller's index of table problem k).  Every
// problem is cut as fginn32_geometry(n1, n2, dim, 0) cuts it alone: its S and tps, whatever G is.
int fginn32_kernel_width(int dim);
int fginn32_group_geometry(int n1, const int *n2, int G, int dim, F32Group &g, int *prob);
// keys: [first[np]][n1][4]; top4: [np][n1][4]
void launch_fginn32_group_topk(hipStream_t s, const F32Group &g, const float *queries, int n1, unsigned long long *keys,
                               unsigned long long *top4);
// open / closed: uend[np - 1] entries sorted by problem, closed = {all ones, 0} on entry; g.ubeg / uend / rfirst are set
void launch_fginn32_group_resolve(hipStream_t s, const F32Group &g, const float *queries, const F32Open *open, double contrDistSq,
                                  F32Closed *closed);
// dst: n rows of DK floats at their place in a stored slot; *flag |= bit for a value outside the matcher's contract
void launch_fginn32_pack_rows(hipStream_t s, const float *src, int n, int dim, int DK, float *dst, unsigned *flag, unsigned bit);
// LIOP (kernels_liop.hip).  One neighbour sample of a measurement pixel: floor and fraction of neighSamplesX / Y (liop.c:376-395,
// 503-507), built by the host with libm (engine_liop.hip: liop_tables)
struct LiopSample { double wx, wy; int ix, iy; };
static_assert(sizeof(LiopSample) == 24, "sample table entries are 24 bytes");
void launch_liop(hipStream_t s, const float *patches, int n, float *out, const DescJob *jobs, const unsigned short *pixels,
                 const LiopSample *samples, unsigned *exactCount, int *dbgPath, int *dbgPerm);
// SURF (kernels_surf.hip).  The constants of (patchSize = 41, mrSize), built by the host with libm (engine_surf.hip: surf_tables):
// sample_x of k = -12 .. 11, sample_y of l = -12 .. 11, the Haar size, gauss_s2 per sub-region, gauss_s1 per sub-region and sample
struct SurfTab { int sx[24], sy[24]; int haar, pad[3]; float w2[16]; float w1[16 * 81]; };
static_assert(sizeof(SurfTab) == (24 + 24 + 4 + 16 + 16 * 81) * 4, "the SURF table is a dense block of words");
void launch_surf(hipStream_t s, const float *patches, int n, float *out, const DescJob *jobs, const SurfTab *tab);
// DAISY (kernels_daisy.hip).  The constants of (rad, radq, thq) at patchSize 41 and histq 8, built by the host with libm
// (engine_daisy.hip: daisy_tables): the 5-tap kernel, (kos, zin) per layer, the 1 + radq filters (0: the smoothing of the layers,
// 1 + r: cube r - 1 -> cube r), and per grid point its cube, its state, the index of pixel A and the bilinear weights w0 .. w3.
// A row of taps is DAISY_TAP_PAD zeros, the fsz taps, then zeros: k_daisy reads windows of 14 entries in steps of 8
constexpr int DAISY_MAX_PTS = MODSX_DAISY_MAX_DIM / 8, DAISY_MAX_TAPS = MODSX_DAISY_MAX_TAPS, DAISY_TAP_PAD = 6, DAISY_TAP_ROW = 72;
static_assert((DAISY_MAX_TAPS + DAISY_TAP_PAD + 7) / 8 * 8 + DAISY_TAP_PAD <= DAISY_TAP_ROW, "the last window stays inside the row");
struct DaisyTab {
  int npts, nfilt, dim, pad;
  float k5[8], kos[8], zin[8];
  int fsz[4];
  int cube[DAISY_MAX_PTS + 3], state[DAISY_MAX_PTS + 3], base[DAISY_MAX_PTS + 3];
  float w[(DAISY_MAX_PTS + 3) * 4];
  float taps[4 * DAISY_TAP_ROW];
};
void launch_daisy(hipStream_t s, const float *patches, int n, float *out, const DescJob *jobs, const DaisyTab *tab, int nrmType);
// The SURF detector (kernels_surfdet.hip; OpenSURF's FastHessian on a whole view).  Every kernel reads a job table in device memory,
// one SdJob per image, and finds its (job, part) through a table of workgroup runs, so a view set is one launch set.
constexpr int SD_MAX_LAYERS = MODSX_SURFDET_MAX_LAYERS, SD_ROWS_PER_WG = 16, SD_TILE = 256;
struct SdLayer { int w, h, step, filter; unsigned long long ofs; };   // ofs: the plane's offset in the response (f32) and laplacian (u8) arenas
struct SdJob { const float *src; float *integ; int rows, cols, nLayers, pad; SdLayer L[SD_MAX_LAYERS]; };
// a run of workgroups that starts at workgroup blk0: 16 rows / 64 columns of image `job` (a, b unused), SD_TILE pixels of its layer a, or
// SD_TILE raster positions of the t layer of (octave a, interval b)
struct SdSeg { int job, a, b, blk0; };
struct SdPoint { float x, y, scale; int laplacian; };                  // an Ipoint as getIpoints pushes it
struct SdExt { int job, o, i, r, c, accepted, laplacian, pad; double dD[3], H[6], x[3]; };   // modsx_debug_surfdet: one raw extremum
void launch_surfdet_integral(hipStream_t s, const SdJob *jobs, const SdSeg *rowSegs, int nRowSegs, int rowBlocks, const SdSeg *colSegs,
                             int nColSegs, int colBlocks);
void launch_surfdet_responses(hipStream_t s, const SdJob *jobs, const SdSeg *segs, int nsegs, int blocks, float *resp, unsigned char *lap);
// the first pass over the t layers (flags [tiles][SD_TILE]: bit 0 extremum, bit 1 accepted; counts [tiles] int2), then the exclusive
// scan (offs [tiles + 1] int2; jobStart [nj + 1] int2 = offs at tile0[j])
void launch_surfdet_scan(hipStream_t s, const SdJob *jobs, const SdSeg *segs, int nsegs, int tiles, const float *resp,
                         const unsigned char *lap, float thresh, unsigned char *flags, int *counts, int *offs, const int *tile0, int nj,
                         int *jobStart);
// the second pass: points [capPts] and / or ext [capExt] in push order (either may be null)
void launch_surfdet_emit(hipStream_t s, const SdJob *jobs, const SdSeg *segs, int nsegs, int tiles, const float *resp,
                         const unsigned char *lap, const unsigned char *flags, const int *offs, SdPoint *points, int capPts, SdExt *ext,
                         int capExt);
// The KAZE detector (kernels_kaze.hip; AKAZE's nonlinear scale space and Hessian extrema on a whole view).  Every kernel reads a run
// of KzJob records in device memory, one per image and stage, and finds its image through the records' first workgroups, so a view
// set is one launch per stage.  Stencil tiles are KZ_TW x KZ_TH outputs with a halo of at most KZ_MAX_S; the diffusion step and the
// half-size resize take 64 x 4 pixels per workgroup; the scan takes KZ_TILE raster positions.
constexpr int KZ_MAX_LEVELS = MODSX_KAZE_MAX_LEVELS, KZ_MAX_TAU = MODSX_KAZE_MAX_TAU, KZ_MAX_OCTAVES = 8, KZ_TW = 64, KZ_TH = 16,
              KZ_MAX_S = 8, KZ_TILE = 256, KZ_MAX_BINS = 4096;
enum { KZ_DERIV = 0, KZ_FLOW = 1, KZ_MAX = 2, KZ_HIST = 3 };      // the epilogues of k_kz_first
struct KzJob {
  const float *in0, *in1;      // the planes a stage reads (the diffusion step: Lt, Lflow; the second derivatives: Lx, Ly)
  float *out0, *out1;
  int rows, cols, srows, scols;   // of the output; of the source of the half-size resize
  int s;                       // the derivative distance
  float t0, t1, t2, scale;     // the smoothing taps; (float)(s * s)
  int slot, octave, level;     // the image's index in the launch set
  int blk0, tilesX;            // the first workgroup of the job and its tiles per row
  int pad;
};
struct KzRaw { int slot, level, r, c; float value; };                 // one 3 x 3 maximum of an Ldet plane
struct KzItem { unsigned long long ofs; int cols, y, x, pad; };       // k_kz_gather: the plane's offset in the Ldet arena
void launch_kaze_scale(hipStream_t s, const KzJob *jobs, int njobs, int blocks);
// hist [slots][nbins + 1]: the bits of hmax, then the bins; kinv [slots][KZ_MAX_OCTAVES] = (float)(1.0 / (double)(k * k)) per octave
void launch_kaze_first(hipStream_t s, int mode, const KzJob *jobs, int njobs, int blocks, const float *kinv, unsigned *hist, int nbins);
void launch_kaze_second(hipStream_t s, const KzJob *jobs, int njobs, int blocks);
void launch_kaze_fed(hipStream_t s, const KzJob *jobs, int njobs, int blocks, float tau);
void launch_kaze_half(hipStream_t s, const KzJob *jobs, int njobs, int blocks);
// flags [tiles][KZ_TILE], counts [tiles], then the exclusive scan offs [tiles + 1] and slotStart [nslots + 1] = offs at tile0[slot]
void launch_kaze_scan(hipStream_t s, const KzJob *jobs, int njobs, int tiles, float dthr, float minthr, unsigned char *flags, int *counts,
                      int *offs, const int *tile0, int nslots, int *slotStart);
void launch_kaze_emit(hipStream_t s, const KzJob *jobs, int njobs, int tiles, const unsigned char *flags, const int *offs, KzRaw *raw, int cap);
void launch_kaze_gather(hipStream_t s, const KzItem *items, int n, const float *ldet, float *out);
// the patch-out form of k_describe (kernels_describe.hip): [slot][1681] f32, slot = outIdx (patchByOutIdx) or the job's index
void launch_describe_patch(hipStream_t s, const DescJob *jobs, int n, const ImgRef *imgs, const float *grid, const int *needTab,
                           const float *coordTab, const unsigned short *maskIdx, int nmask, int photoNorm, float *patchOut,
                           int patchByOutIdx);
// the raw-histogram form of k_describe: raw[outIdx][128] f32 = (float)vec[i] of the doNorm = false functor, stored (accumulate = 0)
// or added in f32 to what is there (accumulate = 1)
void launch_describe_raw(hipStream_t s, const DescJob *jobs, int n, const ImgRef *imgs, const float *grid, const int *needTab,
                         const float *coordTab, const float *mask, const unsigned short *maskIdx, int nmask, const float *oTab,
                         const int *bins, const double *wts, int photoNorm, float *raw, int accumulate, unsigned *orderedCnt);
// SIFTnorm(std::vector<float>&) over [n][128] f32 rows (kernels_dsp.hip); out may be rows; 4-byte alignment suffices
void launch_sift_norm_f32(hipStream_t s, const float *rows, int n, double maxBin, float *out);

// ---- CLAHE (kernels_clahe.hip, engine_clahe.hip): cv::CLAHE::apply of OpenCV 2.4.9 on the gray f32 image ----
constexpr int CLAHE_BINS = 256;
constexpr int CLAHE_MAX_TILES = 256;      // MODSX_CLAHE_MAX_TILES: the image's LUT table (tiles x 256 B) is one workgroup's LDS, 64 KiB
constexpr int CLAHE_STRIP_PX = 4096;      // a histogram workgroup takes whole tile rows up to this many pixels ...
constexpr int CLAHE_MAX_STRIPS = 256;     // ... and a tile is never cut into more strips than this
constexpr int CLAHE_APPLY_PX = 4096;      // consecutive pixels (row-major) one workgroup of k_clahe_apply maps
// what the three launches need of one image; one entry per image of a batch, read from a device table
struct ClaheImg {
  const float *src;
  float *dst;
  long long partOfs;      // first [256]-int partial histogram of the image: (partOfs + tile * strips + strip) * 256
  long long lutOfs;       // first tile of the image in the LUT table: (lutOfs + tile) * 256 bytes
  int rows, cols, tileW, tileH;
  int strips, stripRows;  // row strips per tile and the tile rows in each (the last one may be shorter)
  int clipLimit, applyBlocks;
  float lutScale;
  int vec;                // src and dst are 16-byte aligned: quads of four consecutive pixels move as one access
};
void launch_clahe_hist(hipStream_t s, const ClaheImg *imgs, int n, int tx, int ty, int maxStrips, int *partials);
// dbgHist (optional): [all tiles][256] the summed counts before clipping
void launch_clahe_lut(hipStream_t s, const ClaheImg *imgs, int n, int tiles, int variant, const int *partials, unsigned char *lut,
                      int *dbgHist);
void launch_clahe_apply(hipStream_t s, const ClaheImg *imgs, int n, int tx, int ty, int variant, int maxBlocks, const unsigned char *lut);

// ---- the learned-descriptor front end (kernels_caffe.hip, engine_caffe.hip): the "CAFFE" branch, imagerepresentation.cpp:1343-1534 ----
// one region: the f32 arguments interpolate() is called with (the products with curr_sc made), and whether
// interpolateCheckBorders is true for them on the planes of the call
struct CaffeJob { float x, y, a11, a12, a21, a22, sc; int touch; };
static_assert(sizeof(CaffeJob) == 32, "caffe jobs are 32 bytes");
constexpr int CAFFE_MAX_PATCH = 255;      // odd patch sizes 1 .. 255: one to four wavefronts of rows
constexpr int CAFFE_COLS = 64;            // columns of the patch a workgroup samples before it stores them: one store row per wavefront
constexpr int CAFFE_NORM_ROWS = 16;       // rows of a k_caffe_norm wavefront (one lane each sums a row) ...
constexpr int CAFFE_NORM_COLS = 128;      // ... and the columns of the LDS tile they move through
constexpr int CAFFE_MAX_DIM = 4096;
// what a launch over P x P patches looks like (modsx_debug_caffe_geometry): wavefronts per workgroup (one lane per patch row),
// column chunks, columns per chunk, LDS byte stride of a tile row (a multiple of 4, an odd number of dwords), LDS bytes per plane
struct CaffeGeo { int waves, chunks, chunkCols, stride, planeBytes; };
inline CaffeGeo caffe_geometry(int P) {
  CaffeGeo g;
  g.waves = (P + 63) / 64;
  g.chunkCols = P < CAFFE_COLS ? P : CAFFE_COLS;
  g.chunks = (P + g.chunkCols - 1) / g.chunkCols;
  const int dw = (g.chunkCols + 3) / 4;
  g.stride = 4 * (dw | 1);
  g.planeBytes = g.stride * P;
  return g;
}
// planes: 1 (gray, the byte goes to all three channels) or 3 (B, G, R) images of rows x cols; out [n][3][P][P] f32 (4-byte aligned);
// flags [n] u8 (may be null): bit 0 = jobs[i].touch, bit 1 = a sample fell outside the plane
void launch_caffe_patches(hipStream_t s, const CaffeJob *jobs, int n, const float *p0, const float *p1, const float *p2, int nplanes,
                          int rows, int cols, int P, float m0, float m1, float m2, float *out, unsigned char *flags);
// norm: MODSX_CAFFE_NORM_*; rows / out [n][dim] f32 (4-byte aligned), out may be rows
void launch_caffe_norm(hipStream_t s, const float *rows, int n, int dim, int norm, float *out);

}  // namespace mx

namespace mx {
// experiment aid (builds with -DMODSX_DUP_BUILD only; tools/ab_dup.sh): MODSX_DUP=<bit mask of KClass> launches the kernels of those
// classes twice, which prices a kernel under the bench's 16 streams without changing any result (the launches are idempotent)
#ifdef MODSX_DUP_BUILD
int dup_count(int cls);
#define MX_DUP(cls) for (int dupLeft_ = mx::dup_count(cls); dupLeft_ > 0; dupLeft_--)
#else
#define MX_DUP(cls)
#endif
enum KClass { K_BLUR_HESS = 0, K_HESSIAN, K_RESIZE, K_NMS, K_BAUMBERG, K_ORIENT, K_PATCH_SAMPLE, K_BLUR_ROWS, K_DESCRIBE,
              K_MATCH, K_GRAY, K_WARP, K_VIEW_BLUR, K_BLUR_COLS, K_MATCH_SWEEP1, K_MATCH_DB, K_NCLASS };
struct Profiler {
  bool enabled = false;
  std::vector<hipEvent_t> evA, evB;
  std::vector<int> cls;
  size_t used = 0;
  double ms[K_NCLASS] = {0};
  double work[K_NCLASS] = {0};   // algorithmic bytes (flops for K_MATCH)
  long launches[K_NCLASS] = {0};
};
}  // namespace mx

namespace mx {
// measurement hook (modsx_describe_counters): cumulative plan of describe_batch per context (describe_plan.cpp books the chunks), in
// the order of include/modsx.h
enum DescCounter { DC_CALLS = 0, DC_CHUNKS, DC_MAX_CHUNKS, DC_CHUNKS_MID_IMAGE, DC_CHUNKS_LATER_IMAGE, DC_JOBS, DC_DIRECT_JOBS,
                   DC_FUSED_WINDOWS, DC_LDS_ROW_TILES, DC_LDS_COL_TILES, DC_SAMPLE_TILES, DC_GLOBAL_ROW_TILES, DC_GLOBAL_COL_TILES,
                   DC_CLAMPED_WINDOWS, DC_N,
                   // behind the planner's: k_describe workgroups that took the ordered gather, counted on the device
                   // (modsx_ctx::dDescOrdered) and read by modsx_describe_counters alone
                   DC_ORDERED_WG = DC_N, DC_ALL };
// measurement hook (modsx_detect_counters): what the scale-space front end launched on a context since modsx_create, in the order
// of include/modsx.h.  Host-side increments next to the launches; DT_LAST_* describe the context's last scan / candidate set.
enum DetectCounter { DT_BLUR_TH16 = 0, DT_BLUR_TH32, DT_BLUR_R1, DT_BLUR_R8 = DT_BLUR_R1 + 7, DT_HESSIAN, DT_RESIZE, DT_SCAN_OCTAVE,
                     DT_SCAN_LEVEL, DT_NMS_FLUSHES, DT_LAST_JOBS, DT_LAST_TILES, DT_LAST_ACCEPTED, DT_SECOND_COPIES, DT_N };
}  // namespace mx

struct modsx_db { mx::DbSet set; };

struct modsx_image {
  float *d;
  int rows, cols;
  bool owned;
};

struct modsx_ctx {
  int dev;
  hipStream_t stream;
  mx::Pyramid pyr[mx::MAXB];
  mx::DevBuf candSort, candOut;   // device-side detection order: keys / indices / hash table / temp storage, and the ordered survivors
  size_t lastSurvivors = 0;
  mx::DevBuf nmsJobs, cand, counter, affJobs, affOut, oriJobs, oriOut, descJobs, tilePrefix, taps, imgRefs, scratchA, scratchB,
      descF[mx::MAXB], descU8[mx::MAXB], descAllF[2], descAllU8[2], descAllU8b[2], descCls[2][4][2], descU8x[3][mx::MAXB], shardLocal, pos2, matchRows, matchWork, dbSel, misc, viewTmp[2], viewTaps, viewJobs, viewImg[mx::MAXB], scratchC, needTab, coordTab, tileJob, blurTiles, nmsQueue, rowStarts;
  mx::ImgRef imgRefsHost[mx::MAXB];   // what imgRefs holds on the device
  mx::PinBuf hDescB;           // second staging blob of describe_batch: chunk k + 1 is prepared while chunk k runs
  hipEvent_t descEv[2];
  bool descEvPending[2] = {false, false};
  bool descByEvent[2] = {true, true};
  unsigned descMark[2] = {0, 0};   // ... as sequence numbers of the context's flag word (ctx_mark) when the runtime's waits are not used
  unsigned *hFlag = nullptr;   // pinned word the stream's flag kernel writes (ctx_sync, engine.hip)
  unsigned flagSeq = 0;        // last sequence number issued
  bool waitRuntime = true;     // how the call in progress waits and copies (latched by CtxBusy from MODSX_HOST_WAIT / the CPU load)
  mx::PinBuf hCand, hAff, hOri, hDesc, hMisc, hNms, hMatch, hViewTaps, hViewJobs, hMser, hRefs;
  // constant tables on device
  float *dSmmMask = nullptr;   // 19x19 computeGaussMask
  int baumResident = 0;        // baumberg_resident_waves() of this context's device, asked at the first Baumberg launch (-1: no answer)
  int smmW = 0;
  std::vector<uint64_t> candKeys, candKeys2, candClaim;   // detection-order sort + octaveMap claim scratch (host)
  std::vector<uint32_t> candOrder, candOrder2;
  float *dOriMask = nullptr;   // values of the 41x41 circular mask (sigma = 41/3) at the ORI_NV listed pixels
  unsigned short *dOriIdx = nullptr;   // their index in the kernel's padded 44-column patch, raster order
  float *dSiftMask = nullptr;  // 41x41 circular mask, sigma2 = 0.9 r^2
  unsigned short *dSiftMaskIdx = nullptr;  // raster-ordered indices of the pixels with mask > 0
  int nSiftMask = 0;
  double *dAtan = nullptr;
  unsigned char *dOriBinTab = nullptr;   // histogram bin of every atan2LUT angle (ATAN_CASES entries)
  float *dSiftOTab = nullptr;            // fractional SIFT orientation bin of every atan2LUT angle
  int *dSiftBins = nullptr;    // bin0[41], bin1[41]
  double *dSiftW = nullptr;    // w0[41], w1[41]
  double timings[6];
  mx::Profiler prof;
  size_t lastCandCount = 0;    // scale-space candidates of the context's last launch set (sizes the speculative download)
  const mx::DbSet *fginnDb = nullptr;   // modsx_set_fginn_db: the fused callers match their RootSIFT class against it (useDBforFGINN)
  long descCnt[mx::DC_N] = {0};   // modsx_describe_counters: what describe_batch planned on this context since modsx_create
  unsigned *dDescOrdered = nullptr;   // device words: k_describe workgroups (SIFT and raw forms) that took the ordered gather, and
                                      // [1] those of them that the slim form handed to its redo launch
  bool descSlim = true;               // MODSX_DESCRIBE_SLIM=0 (read when the context is created): today's kernel for every launch
  long descSlimCnt[2] = {0, 0};       // modsx_describe_slim_counters: SIFT launch sets that took the slim form / the full kernel
  unsigned descRedoSeen = 0;          // last reading of dDescOrdered[1] and the sum of the readings' differences
  long descRedoTotal = 0;
  unsigned descOrderedSeen = 0;       // its last reading, and the sum of the readings' differences (the word may wrap)
  long descOrderedTotal = 0;
  long detCnt[mx::DT_N] = {0};    // modsx_detect_counters: what the pyramid and the extrema scan launched on this context
  double hammingMs[2] = {0, 0};   // under modsx_profile: event times of the last Hamming search's packing and search launches
  double fginn32Ms[2] = {0, 0};   // the same for the last f32 FGINN search (or L1 search on byte rows): packing, top-4 sweep + k_f32_merge
  // the patch descriptors LIOP, SURF and DAISY (engine_patchdesc.hip): the patches of one sub-batch (at most 64 MiB), and the
  // descriptors (or the patches of modsx_extract_patches) on their way to a host caller.  Calls are serialised and copy their rows
  // out before they return, so one of each serves all of them
  mx::DevBuf patchBuf, patchOut;
  // LIOP (engine_liop.hip): the measurement pixels + sample table (built at the first LIOP call), debug rows on their way to the
  // host, the exact-path counter word
  mx::DevBuf liopTab, liopDbg, liopCnt;
  long liopCounters[4] = {0, 0, 0, 0};   // modsx_liop_counters: calls, regions, regions on the exact path, sub-batches
  // DSP-SIFT (engine_dsp.hip): rows on their way from / to the host
  mx::DevBuf dspRows;
  long dspCounters[3] = {0, 0, 0};       // modsx_dsp_counters: calls, regions, scale passes launched
  // SURF (engine_surf.hip): the tables of the mrSize values seen last (a slot is refilled round robin)
  static constexpr int SURF_TABS = 4;
  mx::DevBuf surfTab[SURF_TABS];
  double surfTabMr[SURF_TABS] = {0, 0, 0, 0};   // 0: the slot is empty (mrSize is positive)
  int surfTabNext = 0;
  long surfCounters[3] = {0, 0, 0};      // modsx_surf_counters: calls, patches, sub-batches
  // DAISY (engine_daisy.hip): the tables of the (rad, radq, thq) triples seen last (a slot is refilled round robin)
  static constexpr int DAISY_TABS = 4;
  mx::DevBuf daisyTab[DAISY_TABS];
  int daisyTabKey[DAISY_TABS] = {0, 0, 0, 0};   // rad << 16 | radq << 8 | thq; 0: the slot is empty
  int daisyTabNext = 0;
  long daisyCounters[3] = {0, 0, 0};     // modsx_daisy_counters: calls, patches, sub-batches
  // the SURF detector (engine_surfdet.hip): integral images, response and laplacian planes, the scan's flags / counts / offsets, the
  // job and run tables, the points (and, for the debug tap, the raw extrema) of one launch set
  mx::DevBuf sdInteg, sdResp, sdLap, sdFlags, sdCounts, sdTab, sdPoints, sdExt;
  mx::PinBuf sdHost, sdBack;
  long sdCounters[5] = {0, 0, 0, 0, 0};  // modsx_surfdet_counters: calls, images, extrema found, points accepted, buffer regrows
  // the KAZE detector (engine_kaze.hip): the per-level scratch planes and the Ldet planes of one launch set, the job tables, the
  // histograms, the scan's flags / counts / offsets, the raw maxima and the gather's items and values
  mx::DevBuf kzPlanes, kzLdet, kzTab, kzHist, kzFlags, kzCounts, kzRaw, kzItems, kzNine;
  mx::PinBuf kzHost, kzBack;
  // modsx_kaze_counters: calls, images, kernel launches, diffusion steps launched, host waits, raw maxima, survivors of the filter
  // passes, keypoints, microseconds the host spent in the filter passes and the refinement
  long kzCounters[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  // external affine adaptation (engine_detect.hip: affine_shape_batch), modsx_affshape_counters: calls, regions in, regions the
  // border test refused, regions launched, regions converged, launches
  long affshapeCounters[6] = {0, 0, 0, 0, 0, 0};
  // CLAHE (engine_clahe.hip): the per-image table, the strip partials, the LUT table and the debug tap's summed histograms of one
  // launch set; modsx_clahe_counters: calls, images, tiles, strips, pixels, launches
  mx::DevBuf claheTab, clahePart, claheLut, claheDbg;
  mx::PinBuf claheHost;
  long claheCounters[6] = {0, 0, 0, 0, 0, 0};
  double claheMs[3] = {0, 0, 0};   // under modsx_profile: event times of the last CLAHE call's three launches
  // the learned-descriptor front end (engine_caffe.hip): the job table, the flags and, for a host caller, the blob or the rows of
  // one call; modsx_caffe_counters: calls, regions, regions on the border branch, launches
  mx::DevBuf caffeJobs, caffeFlags, caffeOut;
  long caffeCounters[4] = {0, 0, 0, 0};
  // float classes of stored representations (engine_reps_f32.hip): dense rows of a device extractor on their way into a slot, and
  // modsx_fginn32_group_counters: grouped launch sets, problems in them, queries sent to resolve, resolve launches
  mx::DevBuf repStage;
  long f32GroupCounters[4] = {0, 0, 0, 0};
  // binary classes (engine_reps_bin.hip), modsx_hamming_group_counters: grouped launch sets, problems in them, rows packed by
  // appends, pack launches issued at match time (stored matches issue none)
  long hamGroupCounters[4] = {0, 0, 0, 0};
  int busyDepth = 0;           // nesting of mx::CtxBusy on this context (its driving thread only)
  int shardLane = 0;           // lane of the rank's communicator this context issues its collectives on (engine_shard.hip)
  modsx_ctx *peer = nullptr;   // second stream + buffers, created on demand: the two images of a multi-view pair run side by side
  modsx_ctx *half = nullptr;   // a lone pair: the second part of an image's views runs here (accumulate_views)
  mx::DevBuf halfDesc[4];      // ... and writes its descriptors (one buffer per descriptor class of the step) here until the first part's count is known
  void *worker = nullptr;      // CtxWorker: the host thread that drives this context when it is a peer / half (engine_views.hip)
};

namespace mx {
inline void book_blur(modsx_ctx *c, const BlurLaunch &g) {
  if (!g.th) return;
  c->detCnt[g.th == 32 ? DT_BLUR_TH32 : DT_BLUR_TH16]++;
  c->detCnt[DT_BLUR_R1 + g.R - 1]++;
}
}  // namespace mx
