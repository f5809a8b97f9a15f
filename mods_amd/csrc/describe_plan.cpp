// describe_plan.cpp -- the planner of the description stage (describe_plan.hpp): host arithmetic only.
#include <math.h>
#include <algorithm>
#include "describe_plan.hpp"

namespace mx {

// DescribeRegions<SIFTDescriptor>, synth-detection.hpp:186-224.  The two branches keep the reference's types: fast extraction
// computes in f64 and narrows at the end, the other rounds ceil(s * mrSize) to f32 first.
int describe_window(double s, double mrSize, int fast, float *i2pOut) {
  if (fast) {
    if (i2pOut) {
      double mrScale = (double)mrSize * s;
      int patchImageSize = 2 * int(mrScale) + 1;
      double i2pd = double(patchImageSize) / (double)DESC_PATCH;
      float curr_sc = i2pd;
      *i2pOut = curr_sc;
    }
    return 0;
  }
  float mrScale = (float)ceil(s * mrSize);
  int patchImageSize = 2 * int(mrScale) + 1;
  float i2p = float(patchImageSize) / float(DESC_PATCH);
  if (i2pOut) *i2pOut = i2p;
  return i2p > 0.4 ? patchImageSize + 2 : 0;
}

// tile shapes of the LDS blur kernels: <= BLUR_OUT outputs and <= BLUR_LDS floats per workgroup
static void size_tiles(int P, DescSizePlan &sp) {
  const std::vector<int> &need = sp.need;
  const int BLUR_LDS = MODSX_SR_WIN, BLUR_LDS_C = MODSX_BLUR_LDS_C, R = sp.ksize >> 1, NP2 = 2 * ((sp.NC + 1) / 2);
  const int cap = 2048 / NP2, capC = 4096 / NP2;
  // the row filter pairs needed columns (2m, 2m+1); they are neighbours in the window by construction
  // (x0, x0 + 1 of one sample, or a contiguous range) -- if ever not, the job takes the global-memory kernel
  bool pairs = true;
  for (int a = 0; a + 1 < sp.NC; a += 2) pairs = pairs && need[a + 1] == need[a] + 1;
  sp.rows0 = pairs ? std::min(cap, BLUR_LDS / (P + 2 * R)) : 0;
  if (sp.rows0 < 2) sp.rows0 = 0;
  sp.clamped = sp.rows0 > 32 && sp.rows0 < 48 && sp.rows0 < P;
  if (sp.clamped) sp.rows0 = 32;   // the fused sampling kernel parks 8 columns x <= 32 rows or 4 x <= 64 (MODSX_SR_HALF)
  sp.ro1 = 0;
  const int LS = sp.NC <= 64 ? 64 : 96;   // LDS row stride of the column filter
  for (int ro = std::min(capC, sp.NC); ro >= 2 && !sp.ro1 && sp.NC <= 96; ro--) {
    int span = 0;
    for (int a = 0; a < sp.NC; a += ro) span = std::max(span, need[std::min(a + ro, sp.NC) - 1] - need[a] + 2 * R + 1);
    if (span * LS <= BLUR_LDS_C) sp.ro1 = ro;
  }
  // a window that is one row tile, with <= 64 needed columns and <= 80 block rows (kernels_describe.hip: FC_LS,
  // FC_ROWS): the fused sampling kernel runs the column filter too
  if (sp.rows0 >= P && sp.NC <= 64 && P + 2 * R <= MODSX_FC_ROWS) sp.ro1 = -1;
}

int describe_size_plan(int P, DescSizePlan &sp) {
  const float i2p = float(P - 2) / float(DESC_PATCH);
  float sigma = 1.5f * i2p;
  sp.ksize = blur_ksize(sigma);
  if (sp.ksize > 512) { set_error("descriptor window too large (blur kernel > 512 taps)"); return MODSX_ERR_ARG; }
  sp.taps = gaussian_kernel(sp.ksize, sigma);
  // coordinates of interpolate(smoothed, P/2, P/2, i2p, 0, 0, i2p, patch41): f32 running sums
  // (helpers.cpp:563-585); rows and columns run the same recurrence (a12 = a21 = 0, ofsx = ofsy)
  const float o = (float)(P >> 1);
  sp.touch = check_borders_host(P, P, o, o, i2p, 0.f, 0.f, i2p, 41, 41) ? 1 : 0;
  float *W = sp.coord;
  {
    float rx = o - (float)20 * 0.f;
    float WX = rx - (float)20 * i2p;
    for (int q = 0; q < 41; q++) { W[q] = WX; WX += i2p; }
  }
  int x0[41], valid[41];
  std::vector<int> &need = sp.need;
  need.clear();
  for (int q = 0; q < 41; q++) {
    if (!sp.touch) {
      int x = (int)W[q];
      x = x < 0 ? 0 : (x > P - 2 ? P - 2 : x);
      x0[q] = x; valid[q] = 1;
    } else {
      int x = (int)floorf(W[q]);
      valid[q] = (W[q] >= 0 && x < P - 1) ? 1 : 0;
      x0[q] = valid[q] ? x : 0;
    }
    if (valid[q]) { need.push_back(x0[q]); need.push_back(x0[q] + 1); }
  }
  std::sort(need.begin(), need.end());
  need.erase(std::unique(need.begin(), need.end()), need.end());
  if (need.empty()) need.push_back(0);
  sp.NC = (int)need.size();
  for (int q = 0; q < 41; q++) {
    int i0 = 0, i1 = 0;
    if (valid[q]) {
      i0 = (int)(std::lower_bound(need.begin(), need.end(), x0[q]) - need.begin());
      i1 = (int)(std::lower_bound(need.begin(), need.end(), x0[q] + 1) - need.begin());
    }
    int *e = sp.sampleIdx + 4 * q;
    e[0] = i0; e[1] = i1; e[2] = x0[q]; e[3] = valid[q];
  }
  size_tiles(P, sp);
  return MODSX_OK;
}

// the tables of a window size behind the chunk's tables: taps | needed columns, then the 41 x 4 sample table | coordinates
static DescSizeRef append_size(const DescSizePlan &sp, DescChunkPlan &cp) {
  DescSizeRef r;
  r.ksize = sp.ksize; r.NC = sp.NC; r.touch = sp.touch; r.rows0 = sp.rows0; r.ro1 = sp.ro1; r.clamped = sp.clamped;
  r.tapOfs = (int)cp.taps.size();
  cp.taps.insert(cp.taps.end(), sp.taps.begin(), sp.taps.end());
  r.needOfs = (int)cp.needTab.size();
  cp.needTab.insert(cp.needTab.end(), sp.need.begin(), sp.need.end());
  cp.needTab.insert(cp.needTab.end(), sp.sampleIdx, sp.sampleIdx + DESC_PATCH * 4);
  r.coordOfs = (int)cp.coordTab.size();
  cp.coordTab.insert(cp.coordTab.end(), sp.coord, sp.coord + DESC_PATCH);
  return r;
}

DescCursor describe_windows(DescBatch &b) {
  host_parallel_light(b.n, [&](int i) {
    b.winP[i].resize(b.regs[i].size());
    for (size_t r = 0; r < b.regs[i].size(); r++) b.winP[i][r] = describe_window(b.regs[i][r].det_kp.s, b.mrSize, b.fast);
  });
  DescCursor c = {0, 0};
  while (c.img < b.n && b.regs[c.img].empty()) c.img++;
  return c;
}

// Which regions the chunk takes: a light sequential walk over the window sizes, which builds the tables of a size when it first
// appears.  The chunk ends before the window that would overflow the arena, unless it is still empty.  [beg, end) per image.
static int walk_chunk(const DescBatch &b, DescCursor from, size_t arenaFloats, DescChunkPlan &cp, size_t *beg, size_t *end) {
  const int n = b.n;
  for (int q = 0; q < n; q++) { beg[q] = end[q] = 0; }
  bool full = false;
  int i = from.img;
  size_t r = from.reg, count = 0;
  cp.windowFloats = 0;
  for (; i < n && !full; i++, r = 0) {
    beg[i] = r;
    for (; r < b.regs[i].size(); r++) {
      const int P = b.winP[i][r];
      if (P > 0) {
        if (cp.sizes.find(P) == cp.sizes.end()) {
          DescSizePlan sp;
          const int prc = describe_size_plan(P, sp);
          if (prc) return prc;
          cp.sizes.insert({P, append_size(sp, cp)});
        }
        const size_t needA = (size_t)P * P;
        if (cp.windowFloats + needA > arenaFloats && count) { full = true; break; }
        cp.windowFloats += needA;
      }
      count++;
    }
    end[i] = r;
    if (full) break;
  }
  // (i, r) = first region that did not fit, or i == n
  if (full) cp.next = {i, r}; else cp.next = {n, 0};
  return MODSX_OK;
}

// the job records of regions [beg, end) of every image, in (image, region) order: one pool task per image
static void write_jobs(const DescBatch &b, const DescChunkPlan &cp, const size_t *beg, const size_t *end, std::vector<DescJob> &jobs) {
  size_t at[MAXB + 1];
  at[0] = 0;
  for (int q = 0; q < b.n; q++) at[q + 1] = at[q] + (end[q] - beg[q]);
  jobs.resize(at[b.n]);
  host_parallel_light(b.n, [&](int q) {
    for (size_t rr = beg[q]; rr < end[q]; rr++) {
      const modsx_keypoint &k = b.regs[q][rr].det_kp;
      DescJob j;
      memset(&j, 0, sizeof j);
      j.img = q;
      j.outIdx = (int)rr;
      j.x = (float)k.x; j.y = (float)k.y;
      describe_window(k.s, b.mrSize, b.fast, &j.i2p);
      j.P = b.winP[q][rr];
      if (j.P > 0) {
        const DescSizeRef &pi = cp.sizes.find(j.P)->second;
        j.a11 = (float)k.a11; j.a12 = (float)k.a12; j.a21 = (float)k.a21; j.a22 = (float)k.a22;
        j.tapOfs = pi.tapOfs; j.ksize = pi.ksize; j.NC = pi.NC; j.needOfs = pi.needOfs; j.coordOfs = pi.coordOfs;
        j.touch = pi.touch; j.rows0 = pi.rows0; j.ro1 = pi.ro1;
      } else {   // the direct branch: A * imageToPatchScale
        j.a11 = (float)k.a11 * j.i2p; j.a12 = (float)k.a12 * j.i2p; j.a21 = (float)k.a21 * j.i2p; j.a22 = (float)k.a22 * j.i2p;
      }
      jobs[at[q] + (rr - beg[q])] = j;
    }
  });
}

// Launch order of the chunk: by image, then by 64-pixel row band, then by x.  The sampling kernel hands every XCD one
// contiguous eighth of this order (kernels_describe.hip: xcd_chunk), i.e. one part of the images; outIdx keeps every
// descriptor at its region's place, so the reference's list order is untouched.
// (a stable LSD radix sort of one key per job: jobs are generated in (image, outIdx) order, which breaks the ties)
static void sort_jobs(std::vector<DescJob> &jobs) {
  // the key in the high half of a word, the job's position in the low half; sorted by the key's bits alone, the low halves
  // are the order.  MAXB = 32 leaves room: the key needs 31 bits (image 5 | band 10 | x 16) of its 32
  static_assert(MAXB <= 64, "describe job sort key: the image index has 6 bits at the most");
  const size_t nj = jobs.size();
  std::vector<uint64_t> key(nj), key2;
  for (size_t q = 0; q < nj; q++) {
    const DescJob &a = jobs[q];
    // the order only places neighbouring windows on neighbouring workgroups (no result depends on it): whole pixels
    // are enough, and a 32-bit key is three passes instead of six
    const int xi = (int)a.x, yb = (int)a.y >> 6;
    const uint32_t x16 = (uint32_t)(xi < 0 ? 0 : (xi > 65535 ? 65535 : xi));
    const uint32_t band = (uint32_t)(yb < 0 ? 0 : (yb > 1023 ? 1023 : yb));
    key[q] = ((((uint64_t)(uint32_t)a.img << 26) | ((uint64_t)band << 16) | x16) << 32) | (uint32_t)q;
  }
  host_radix_sort_u64(key, key2, 32, 63);
  std::vector<DescJob> sorted(nj);
  for (size_t q = 0; q < nj; q++) sorted[q] = jobs[(uint32_t)key[q]];
  jobs.swap(sorted);
}

// arena offsets of every job in launch order, the five tile prefixes and the chunk's counters
static void layout_chunk(DescChunkPlan &cp) {
  cp.arenaA = cp.arenaB = cp.arenaC = 0;   // arena A only holds the windows that do not take the fused kernel
  cp.rowStarts = 0;                        // the fused ones get their P row starts (float2) instead
  for (DescJob &j : cp.jobs) {
    if (j.P > 0) {
      j.rowOfs = cp.arenaB; j.gridOfs = cp.arenaC;
      if (!j.rows0) { j.scratchOfs = cp.arenaA; cp.arenaA += (size_t)j.P * j.P; }
      else { j.scratchOfs = cp.rowStarts; cp.rowStarts += (size_t)j.P; }
      cp.arenaB += (size_t)j.P * j.NC; cp.arenaC += (size_t)j.NC * j.NC;
    }
    // windows whose row tile fits LDS are sampled by the fused sample + row-filter kernel (arena A is not touched); the
    // others go through k_patch_sample (64 x SAMPLE_COLS tiles) and the global-memory row filter
    cp.pfxSample.push_back(cp.pfxSample.back() + (j.P > 0 && !j.rows0 ? ((j.P + 63) / 64) * ((j.P + 127) / 128) : 0));
    // the blur passes: LDS kernels where a tile fits, k_patch_blur (BLUR_TILE outputs per workgroup) otherwise
    cp.pfxRowL.push_back(cp.pfxRowL.back() + (j.P > 0 && j.rows0 ? (j.P + j.rows0 - 1) / j.rows0 : 0));
    cp.pfxColL.push_back(cp.pfxColL.back() + (j.P > 0 && j.ro1 > 0 ? (j.NC + j.ro1 - 1) / j.ro1 : 0));
    cp.pfxRow.push_back(cp.pfxRow.back() + (j.P > 0 && !j.rows0 ? (j.P * j.NC + 1023) / 1024 : 0));
    cp.pfxCol.push_back(cp.pfxCol.back() + (j.P > 0 && j.ro1 == 0 ? (j.NC * j.NC + 1023) / 1024 : 0));
    cp.cnt[DC_DIRECT_JOBS] += j.P == 0;
    cp.cnt[DC_FUSED_WINDOWS] += j.P > 0 && j.ro1 == -1;
    cp.cnt[DC_CLAMPED_WINDOWS] += j.P > 0 && cp.sizes.find(j.P)->second.clamped;
  }
  cp.slim = !cp.jobs.empty() && cp.cnt[DC_DIRECT_JOBS] == 0;
  cp.cnt[DC_JOBS] += (long)cp.jobs.size();
  cp.cnt[DC_LDS_ROW_TILES] += cp.pfxRowL.back();
  cp.cnt[DC_LDS_COL_TILES] += cp.pfxColL.back();
  cp.cnt[DC_SAMPLE_TILES] += cp.pfxSample.back();
  cp.cnt[DC_GLOBAL_ROW_TILES] += cp.pfxRow.back();
  cp.cnt[DC_GLOBAL_COL_TILES] += cp.pfxCol.back();
}

int describe_plan_chunk(const DescBatch &b, DescCursor from, size_t arenaFloats, DescChunkPlan &cp, HostMark &hm) {
  cp.jobs.clear(); cp.taps.clear(); cp.coordTab.clear(); cp.needTab.clear(); cp.sizes.clear();
  for (std::vector<int> *p : {&cp.pfxSample, &cp.pfxRow, &cp.pfxCol, &cp.pfxRowL, &cp.pfxColL}) p->assign(1, 0);
  cp.arenaA = cp.arenaB = cp.arenaC = cp.rowStarts = 0;
  for (int q = 0; q < DC_N; q++) cp.cnt[q] = 0;
  cp.slim = false;
  // a chunk is counted when its walk begins: a refusal leaves a chunk with no jobs
  cp.cnt[DC_CHUNKS] = 1;
  cp.cnt[DC_CHUNKS_MID_IMAGE] = from.reg > 0;
  cp.cnt[DC_CHUNKS_LATER_IMAGE] = from.img > 0;
  size_t beg[MAXB], end[MAXB];
  const int rc = walk_chunk(b, from, arenaFloats, cp, beg, end);
  if (rc) return rc;
  write_jobs(b, cp, beg, end, cp.jobs);
  hm.mark("desc jobs");
  sort_jobs(cp.jobs);
  hm.mark("desc job sort");
  layout_chunk(cp);
  return MODSX_OK;
}

// the job table, the five tile prefixes and the three small tables travel as ONE pinned blob and one copy: nine
// separate uploads cost nine ~6 us copy kernels per chunk on the stream
DescBlobLayout::DescBlobLayout(const DescChunkPlan &cp) {
  const size_t nj = cp.jobs.size();
  oJobs = 0; oPfx = align_up(nj * sizeof(DescJob), 16); pfxB = align_up((nj + 1) * 4, 16);
  oTaps = oPfx + 5 * pfxB; oNeed = oTaps + align_up(cp.taps.size() * 4, 16); oCoord = oNeed + align_up(cp.needTab.size() * 4, 16);
  oRedo = oCoord + align_up(cp.coordTab.size() * 4, 16) + 16;
  blobB = oRedo + 16;
  devB = blobB + align_up(((nj + 1) / 2) * 4, 16);
}

void describe_fill_blob(const DescChunkPlan &cp, const DescBlobLayout &L, char *hb) {
  const size_t nj = cp.jobs.size();
  memcpy(hb + L.oJobs, cp.jobs.data(), nj * sizeof(DescJob));
  const std::vector<int> *pf[5] = {&cp.pfxSample, &cp.pfxRow, &cp.pfxCol, &cp.pfxRowL, &cp.pfxColL};
  for (int q = 0; q < 5; q++) memcpy(hb + L.pfx(q), pf[q]->data(), (nj + 1) * 4);
  if (!cp.taps.empty()) memcpy(hb + L.oTaps, cp.taps.data(), cp.taps.size() * 4);
  if (!cp.needTab.empty()) memcpy(hb + L.oNeed, cp.needTab.data(), cp.needTab.size() * 4);
  if (!cp.coordTab.empty()) memcpy(hb + L.oCoord, cp.coordTab.data(), cp.coordTab.size() * 4);
  memset(hb + L.oRedo, 0, 16);
}

}  // namespace mx
