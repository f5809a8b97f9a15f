// describe_lanes.hpp -- which lane and slot of the LDS describe kernels (kernels_describe.hip: k_sample_rows_lds,
// k_blur_cols_lds) does which element.  The kernels and the host compile the same rules: the host side
// (modsx_debug_describe_lanes / modsx_debug_describe_lane_map, capi.hip) enumerates them for the CPU tests and counts, per
// window size, the lane slots a build issues against the ones that hold a sample or an output pair.
// Only the assignment of work to lanes lives here; the arithmetic of a sample or a sum does not depend on it.
#pragma once
#include "kmath.hpp"

namespace mx {

// --- sampling: the tap slots of one parked chunk -------------------------------------------------------------------------
// Per row pass a wavefront has `rows` <= 64 rows (lane j walks row j) and parks nc columns of their coordinates at a row
// stride of nc | 1 words: odd, so the lane-per-row writes hit 64 different banks.  The chunk is sized from the rows:
// as many columns as give at most SR_SLOTS x 64 samples, which is also what the park holds (rows * (nc | 1) <= 256 + 64 =
// SR_PARK words per array).  The samples of a chunk are e = r * nc + c, e in [0, rows * nc): lane l of slot u takes e = 64 u + l,
// and only ceil(rows * nc / 64) slots are issued.  r = e / nc is a multiply and a shift: with M = ceil(2^16 / nc),
// e * M >> 16 == e / nc for e * (M * nc - 2^16) < 2^16, and e < 256, M * nc - 2^16 < nc <= 63 (tests/test_describe_lanes_cpu.py
// checks every case).  The product is below 2^24, one v_mul_u32_u24.
constexpr int SR_SLOTS = 4;                        // tap slots in flight per lane: 4 samples, 16 loads
constexpr int SR_PARK = 64 * (SR_SLOTS + 1);       // words per wavefront and coordinate array
constexpr int SR_MAXC = 63;                        // largest chunk (and divisor)

constexpr int sr_chunk_cols(int rows) { return 64 * SR_SLOTS / rows < SR_MAXC ? 64 * SR_SLOTS / rows : SR_MAXC; }   // rows in 1 .. 64
constexpr int sr_stride(int ncFull) { return ncFull | 1; }
constexpr unsigned sr_magic(int nc) { return (65536u + (unsigned)nc - 1u) / (unsigned)nc; }                          // nc in 1 .. 64

// both per-chunk constants come out of one table word (a scalar load in the kernel, no division): index x in 1 .. 64 is
// sr_magic(x) << 8 | sr_chunk_cols(x)
struct SrLaneTable { unsigned w[65]; };
constexpr SrLaneTable sr_lane_table() {
  SrLaneTable t = {};
  for (int x = 1; x <= 64; x++) t.w[x] = sr_magic(x) << 8 | (unsigned)sr_chunk_cols(x);
  return t;
}
MX_HD int sr_table_cols(unsigned w) { return (int)(w & 255u); }
MX_HD unsigned sr_table_magic(unsigned w) { return w >> 8; }

// sample e of a chunk of nc columns: its row and column; the word of its coordinates in the park
MX_HD void sr_sample_rc(unsigned e, int nc, unsigned magic, unsigned &r, unsigned &c) {
#ifdef __HIP_DEVICE_COMPILE__
  r = __umul24(e, magic) >> 16;
  c = e - __umul24(r, (unsigned)nc);
#else
  r = (e * magic) >> 16;
  c = e - r * (unsigned)nc;
#endif
}
MX_HD int sr_slots(int rows, int nc) { return (rows * nc + 63) >> 6; }

// --- filters: rounds of BF_T threads x BF_NQ output pairs ----------------------------------------------------------------
// Pair e of a round that starts at `done` is taken by thread t in slot q with e = done + q * BF_T + t.  Whole rounds run
// while BF_T * BF_NQ pairs remain; in the last round wavefront w only runs the slots q whose first pair exists,
// done + q * BF_T + 64 w < total: bf_live_slots of them (they are the first ones), 0 = the wavefront has nothing left.
constexpr int BF_T = 256, BF_NQ = 4;
MX_HD int bf_live_slots(int rem, int wave) {   // rem = total - done > 0
  const int live = rem - 64 * wave;
  const int k = (live + BF_T - 1) / BF_T;      // (a shift: BF_T is a power of two, and live + 255 < 0 only where k is not used)
  return live <= 0 ? 0 : (k < BF_NQ ? k : BF_NQ);
}

// --- the slot counts of a window size, for the host ----------------------------------------------------------------------
struct LaneCount { long useful, issued, issuedParent; };   // lane slots: holding a sample / pair, issued by this build, by the parent's rule

// one row tile of `nr` rows of a P-wide window: BLUR_W wavefronts, a quarter of the columns each
inline void lanes_count_sampling(int P, int nr, int waves, LaneCount &k) {
  const int cper = (P + waves - 1) / waves;
  for (int w = 0; w < waves; w++) {
    const int cb = w * cper, ce = cb + cper < P ? cb + cper : P;
    if (cb >= ce) continue;
    for (int rb = 0; rb < nr; rb += 64) {
      const int rows = nr - rb < 64 ? nr - rb : 64, ncFull = sr_chunk_cols(rows);
      for (int c0 = cb; c0 < ce; c0 += ncFull) {
        const int nc = ce - c0 < ncFull ? ce - c0 : ncFull;
        k.useful += (long)rows * nc;
        k.issued += 64L * sr_slots(rows, nc);
      }
    }
    // the parent: 8 columns x <= 32 rows per chunk for tiles of up to 32 rows, else 4 x <= 64; four slots per chunk, whatever it held
    const int C = nr <= 32 ? 8 : 4, RG = nr <= 32 ? 32 : 64;
    for (int rb = 0; rb < nr; rb += RG)
      for (int c0 = cb; c0 < ce; c0 += C) k.issuedParent += 64L * 4;
  }
}
// one filter call over `total` output pairs
inline void lanes_count_filter(int total, LaneCount &k) {
  const int round = BF_T * BF_NQ;
  k.useful += total;
  k.issuedParent += (long)((total + round - 1) / round) * round;
  const int done = total / round * round;
  k.issued += done;
  if (total > done)
    for (int w = 0; w < BF_T / 64; w++) k.issued += 64L * bf_live_slots(total - done, w);
}

}  // namespace mx
