// engine_hamming.hip -- MatchFLANNDistance (matching/matching.cpp:607-666) with binary_matcher = linear, binary_dist = HAMMING:
// the exact 2-NN search on the device (kernels_hamming.hip), the reference's record rule on the host (hamming_tentatives, the
// one copy of it), and one binary-descriptor step of mods.cpp:229-415 on caller-supplied regions (match_regions_hamming).
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <string>
#include <vector>
#include "engine_api.hpp"

namespace mx {

static bool hamming_threshold_ok(double t) { return t > 0 && isfinite(t); }

// matching.cpp:647-661 on the search result nn2 = [n1][4] = {first, d(first), second, d(second)}:
// max_distance = (int)(float)distanceThreshold; a query gives a record iff d(first) <= max_distance; records in query order;
// ratio = (double)d1 / (double)d2, 0 / 0 = NaN is returned as such (d1 <= d2, so no infinity occurs)
int hamming_tentatives(const int *nn2, int n1, double distanceThreshold, std::vector<modsx_tentative> &out) {
  out.clear();
  if (!hamming_threshold_ok(distanceThreshold)) {
    set_error("hamming: distanceThreshold must be positive and finite (the reference calls MatchFLANNDistance only with DistanceThreshold > 0)");
    return MODSX_ERR_ARG;
  }
  if (n1 < 0 || (n1 > 0 && !nn2)) { set_error("hamming: bad search result"); return MODSX_ERR_ARG; }
  const float tf = (float)distanceThreshold;
  const int maxDistance = tf >= 2147483648.f ? 2147483647 : (int)tf;      // (the conversion of a larger float is undefined)
  for (int q = 0; q < n1; q++) {
    const int *r = nn2 + 4 * (size_t)q;
    if (r[1] > maxDistance) continue;
    modsx_tentative t;
    t.q = q; t.t0 = r[0]; t.tj = r[2]; t.t1 = r[2];
    t.d1 = (double)r[1]; t.d2 = (double)r[3]; t.d2by2ndcl = t.d2;
    t.ratio = t.d1 / t.d2;
    out.push_back(t);
  }
  return MODSX_OK;
}

// the argument rules every Hamming entry shares; n2 == 1 is refused whatever n1 is: the reference reads a second neighbour that was
// never written
int hamming_check_args(const char *fn, int n1, int n2, int nbytes) {
  const std::string f(fn);
  if (nbytes < 1 || nbytes > MODSX_HAMMING_MAX_BYTES) { set_error(f + ": nbytes must be in [1, MODSX_HAMMING_MAX_BYTES]"); return MODSX_ERR_ARG; }
  if (n1 < 0 || n2 < 0) { set_error(f + ": negative row count"); return MODSX_ERR_ARG; }
  if (n1 > 2000000 || n2 > 2000000) { set_error(f + ": more than 2 000 000 rows on one side"); return MODSX_ERR_ARG; }
  if (n2 == 1) { set_error(f + ": one train row has no second neighbour (MatchFLANNDistance reads one); n2 must be 0 or >= 2"); return MODSX_ERR_ARG; }
  return MODSX_OK;
}

// the raw search on dense [n][nbytes] u8 rows in HBM: nn2 (host, n1 x 4 ints), geo4 (optional) = {tile length in trains, splits
// used, workgroups of k_hamming_2nn, W}.  n1 >= 1, n2 >= 2, arguments checked by the caller.
int hamming_search_device(modsx_ctx *c, const uint8_t *d1, int n1, const uint8_t *d2, int n2, int nbytes, int splits, int *nn2, int *geo4) {
  CtxBusy busy(c);
  const HammingGeo g = hamming_geometry(n1, n2, (nbytes + 3) / 4, splits);
  if (geo4) { geo4[0] = g.tile; geo4[1] = g.S; geo4[2] = g.gx * g.S; geo4[3] = g.W; }
  const size_t rowB = (size_t)n1 * 16;
  if (!c->matchWork.ensure(hamming_workspace_bytes(g, n1)) || !c->matchRows.ensure(rowB) || !c->hMatch.ensure(rowB)) return MODSX_ERR_NOMEM;
  const int rc = search_download(c, [&](hipEvent_t *ev) {      // timed under modsx_profile (tools/bench_hamming.py)
    launch_hamming(c->stream, g, d1, n1, d2, n2, nbytes, c->matchWork.p, (int *)c->matchRows.p, ev);
  }, c->matchRows.p, c->hMatch.p, rowB, c->hammingMs);
  if (rc) return rc;
  c->hamGroupCounters[3] += 2;      // both sides were packed for this call (modsx_hamming_group_counters)
  memcpy(nn2, c->hMatch.p, rowB);
  return MODSX_OK;
}

int match_hamming_device(modsx_ctx *c, const uint8_t *d1, int n1, const uint8_t *d2, int n2, int nbytes, double distanceThreshold,
                         std::vector<modsx_tentative> &out) {
  out.clear();
  int rc = hamming_check_args("modsx_match_hamming", n1, n2, nbytes);
  if (rc) return rc;
  if (!hamming_threshold_ok(distanceThreshold)) return hamming_tentatives(nullptr, 0, distanceThreshold, out);   // its refusal
  if (n1 == 0 || n2 == 0) return MODSX_OK;
  std::vector<int> nn2((size_t)n1 * 4);
  rc = hamming_search_device(c, d1, n1, d2, n2, nbytes, 0, nn2.data(), nullptr);
  if (rc) return rc;
  return hamming_tentatives(nn2.data(), n1, distanceThreshold, out);
}

int upload_row_pair(modsx_ctx *c, DevBuf *buf2, const void *rows1, size_t bytes1, const void *rows2, size_t bytes2) {
  if (!buf2[0].ensure(bytes1) || !buf2[1].ensure(bytes2)) return MODSX_ERR_NOMEM;
  MX_HIP(hipMemcpyAsync(buf2[0].p, rows1, bytes1, hipMemcpyHostToDevice, c->stream));
  MX_HIP(hipMemcpyAsync(buf2[1].p, rows2, bytes2, hipMemcpyHostToDevice, c->stream));
  MX_HIP(hipStreamSynchronize(c->stream));      // the sources are pageable and may be the caller's temporaries
  return MODSX_OK;
}

// rows from the host: dtype 0 = u8, 1 = f32 holding the integers 0..255 (the rule of every other descriptor entry)
int match_hamming_host(modsx_ctx *c, const void *desc1, int n1, const void *desc2, int n2, int nbytes, int dtype, double distanceThreshold,
                       std::vector<modsx_tentative> &out) {
  out.clear();
  int rc = hamming_check_args("modsx_match_hamming", n1, n2, nbytes);
  if (rc) return rc;
  if (dtype != 0 && dtype != 1) { set_error("modsx_match_hamming: dtype must be 0 (u8) or 1 (f32)"); return MODSX_ERR_ARG; }
  if (!hamming_threshold_ok(distanceThreshold)) return hamming_tentatives(nullptr, 0, distanceThreshold, out);
  if (n1 == 0 || n2 == 0) return MODSX_OK;
  const size_t b1 = (size_t)n1 * nbytes, b2 = (size_t)n2 * nbytes;
  std::vector<uint8_t> u1, u2;
  const uint8_t *p1 = (const uint8_t *)desc1, *p2 = (const uint8_t *)desc2;
  if (dtype == 1) {
    u1.resize(b1); u2.resize(b2);
    if (!desc_f32_to_u8((const float *)desc1, b1, u1.data()) || !desc_f32_to_u8((const float *)desc2, b2, u2.data())) {
      set_error("modsx_match_hamming: f32 descriptors must hold the integers 0..255");
      return MODSX_ERR_ARG;
    }
    p1 = u1.data(); p2 = u2.data();
  }
  CtxBusy busy(c);
  if ((rc = upload_row_pair(c, c->descU8, p1, b1, p2, b2))) return rc;
  return match_hamming_device(c, (const uint8_t *)c->descU8[0].p, n1, (const uint8_t *)c->descU8[1].p, n2, nbytes, distanceThreshold, out);
}

// MatchFLANNDistance + DuplicateFiltering + LORANSACFiltering on caller-supplied regions: what match_pair leaves with the match
// stage replaced.  An empty side gives the zeroed result with H = -1 (as modsx_match_reps does for an empty partner).
int match_regions_hamming(modsx_ctx *c, const modsx_region *regs1, const void *desc1, int n1, const modsx_region *regs2, const void *desc2,
                          int n2, int nbytes, int dtype, double distanceThreshold, const modsx_pair_params &pp, modsx_pair_result *res) {
  return match_regions_with(regs1, n1, regs2, n2, pp, res, [&](std::vector<modsx_tentative> &tents) {
    const int rc = hamming_check_args("modsx_match_regions_hamming", n1, n2, nbytes);      // n2 == 1 included: before any work
    return rc ? rc : match_hamming_host(c, desc1, n1, desc2, n2, nbytes, dtype, distanceThreshold, tents);
  });
}

}  // namespace mx
