// describe_plan.hpp -- the host arithmetic of the description stage (describe_plan.cpp): which window a region gets, which
// kernels a window size goes through, which regions one launch set (chunk) takes, its job records in launch order, its arena
// layout and tile prefixes, and where all of that lies in the staged blob.  No HIP runtime call and no context: describe_batch
// (engine.hip) is the driver that stages and launches a plan, modsx_debug_describe_plan (capi.hip) runs the planner alone.
#pragma once
#include <map>
#include <vector>
#include "engine_api.hpp"

namespace mx {

constexpr int DESC_PATCH = 41;   // patchSize: the only one describe_batch accepts

// Window size of a region with scale s: P = patchImageSize + 2 of the smoothed branch, 0 for the direct branch
// (imageToPatchScale <= 0.4, or fast extraction).  *i2p (optional) receives imageToPatchScale as the job record carries it.
int describe_window(double s, double mrSize, int fast, float *i2p = nullptr);

// What a window size P goes through, as a function of P alone: the blur taps, the window columns (= rows) the 41 x 41 resampling
// reads, per sample {index of x0, index of x0 + 1 among them, x0, valid}, the 41 sample coordinates, interpolate()'s border
// branch, and the tile shapes (DescJob::rows0 / ro1; clamped: rows0 was cut to 32).
struct DescSizePlan {
  int ksize, NC, touch, rows0, ro1, clamped;
  std::vector<float> taps;
  std::vector<int> need;
  int sampleIdx[DESC_PATCH * 4];
  float coord[DESC_PATCH];
};
int describe_size_plan(int P, DescSizePlan &sp);   // MODSX_ERR_ARG (and the error text) for a blur kernel of more than 512 taps

// where the tables of a window size lie in the chunk's tables, and the scalars every job of that size copies
struct DescSizeRef { int tapOfs, ksize, needOfs, NC, coordOfs, touch, rows0, ro1, clamped; };

// The regions of one describe_batch call and their window sizes (describe_windows: once per call, one pool task per image).
struct DescBatch {
  const std::vector<modsx_region> *regs;
  int n;
  double mrSize;
  int fast;
  std::vector<int> winP[MAXB];
};
struct DescCursor { int img; size_t reg; };   // first region of the next chunk; img == n: the batch is done
DescCursor describe_windows(DescBatch &b);    // -> the first region of the batch

// One chunk: the regions from a cursor on that fit the window arena, planned as one launch set.
struct DescChunkPlan {
  std::vector<DescJob> jobs;                                  // in launch order, offsets assigned
  std::vector<int> pfxSample, pfxRow, pfxCol, pfxRowL, pfxColL;   // tile prefixes over the jobs (jobs + 1 entries each)
  std::vector<float> taps, coordTab;                          // the tables of every window size of the chunk, size after size
  std::vector<int> needTab;
  std::map<int, DescSizeRef> sizes;                           // per window size P
  size_t arenaA, arenaB, arenaC, rowStarts;                   // floats of the three arenas, float2 row starts of the fused windows
  size_t windowFloats;                                        // all P x P windows of the chunk: its size limit and its algorithmic bytes
  long cnt[DC_N];                                             // what this chunk adds to the counters (DC_CALLS, DC_MAX_CHUNKS: the caller's)
  bool slim;                                                  // no job of the direct branch (P == 0): the SIFT launch may take k_describe's slim form
  DescCursor next;
};
// MODSX_ERR_ARG when a window of the chunk is refused: cnt then holds the chunk and no jobs.  hm: the host-phase marks.
int describe_plan_chunk(const DescBatch &b, DescCursor from, size_t arenaFloats, DescChunkPlan &cp, HostMark &hm);

// The staged blob of a chunk: the job table, the five tile prefixes and the three small tables, each 16-byte aligned, and last the
// count word of the slim form's redo list (16 bytes, staged as zeros: the blob's copy resets it for every launch set).  The list
// itself (one entry per two jobs) lies behind the blob on the device alone: devB >= blobB bytes.
struct DescBlobLayout {
  size_t oJobs, oPfx, pfxB, oTaps, oNeed, oCoord, oRedo, blobB, devB;
  explicit DescBlobLayout(const DescChunkPlan &cp);
  size_t pfx(int q) const { return oPfx + q * pfxB; }         // q: sample, rows, columns, LDS rows, LDS columns
};
void describe_fill_blob(const DescChunkPlan &cp, const DescBlobLayout &L, char *hb);

}  // namespace mx
