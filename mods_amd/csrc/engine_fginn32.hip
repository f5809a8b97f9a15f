// engine_fginn32.hip -- MatchFlannFGINN (matching/matching.cpp:357-461, vector_matcher = linear, ratio^2 < 1) on f32 rows of any
// width: the search on the device (kernels_fginn32.hip), the walk over the neighbours on the host.  The device hands down the four
// nearest keys of every query (32 bytes); the host walks j = 1..3 exactly as the reference does (its f32 division, its f64 positions).
// A walk that is still open behind the fourth neighbour is closed by one more sweep (k_f32_resolve: the nearest train behind the
// fourth that ends the walk, and how many trains do not end it).  That count gives the rank of a passing terminal train exactly, so
// there is no further sweep (kernels_fginn32.hip).  No list of nn neighbours exists anywhere.  The walk itself -- keys, ratio test,
// d_pass, the open / close / emit steps and the record -- is fginn_walk.hpp; this file holds the launches, copies and taps around it.
// The distance (vector_dist of the [Matching] section: L2 or L1) is the chain of the sweep kernels and nothing else: the walk divides
// and compares whatever distances it is handed, squares or not (matching.cpp:437-451).  Under L1, rows that hold the integers 0..255
// at 128 columns have a search of their own on bytes (kernels_fginn_l1.hip) with the same keys, workspace and records.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <string>
#include <vector>
#include "engine_api.hpp"

namespace mx {

bool fginn32_rows_ok(const float *f, size_t n) {
  bool ok = true;
  for (size_t i = 0; i < n; i++) ok = ok && fabs((double)f[i]) <= 1e17;      // NaN fails the comparison
  return ok;
}

// the argument rules every f32 FGINN entry shares, all before any launch
int fginn32_check_args(const char *fn, int n1, int n2, int dim, double ratioT, int nn) {
  const std::string f(fn);
  if (dim < 4 || dim > MODSX_FGINN32_MAX_DIM || dim % 4) {
    set_error(f + ": dim must be a multiple of 4 in [4, MODSX_FGINN32_MAX_DIM] (the linear index's groups of four; the tail loop for other widths is not built)");
    return MODSX_ERR_ARG;
  }
  if (n1 < 0 || n2 < 0) { set_error(f + ": negative row count"); return MODSX_ERR_ARG; }
  if (n1 > 2000000 || n2 > 2000000) { set_error(f + ": more than 2 000 000 rows on one side"); return MODSX_ERR_ARG; }
  if (nn < 2 || nn > MATCH_NN_MAX) { set_error(f + ": nn must be in [2, 256]"); return MODSX_ERR_ARG; }
  if (isnan(ratioT)) { set_error(f + ": ratio is NaN"); return MODSX_ERR_ARG; }
  if (ratioT * ratioT >= 1.0) {
    set_error(f + ": ratio^2 >= 1 (the \"all points\" branch, matching.cpp:397-428) is not built for float rows");
    return MODSX_ERR_ARG;
  }
  return MODSX_OK;
}
int fginn32_check_dist(const char *fn, int dist) {
  if (dist == MODSX_DIST_L2 || dist == MODSX_DIST_L1) return MODSX_OK;
  set_error(std::string(fn) + ": dist must be MODSX_DIST_L2 or MODSX_DIST_L1 (the vector_dist values OpenCV's FLANN takes for float rows)");
  return MODSX_ERR_ARG;
}

static void geo_out(const Fginn32Geo &g, int *geo) {
  geo[0] = g.tile; geo[1] = g.S; geo[2] = g.gx * g.S; geo[3] = g.DK; geo[4] = g.ntiles; geo[5] = g.tilesPerSplit;
}
int fginn32_geometry_report(int n1, int n2, int dim, int splits, int *geo6) {
  geo_out(fginn32_geometry(n1, n2, dim, splits), geo6);
  return MODSX_OK;
}
int fginn_l1_geometry_report(int n1, int n2, int splits, int *geo6) {
  geo_out(fginn_l1_geometry(n1, n2, splits), geo6);
  return MODSX_OK;
}

// d1 / d2: dense rows in HBM -- [n][dim] f32, or with bytes [n][128] u8 (dist is then L1); pos2: [n2][2] f64 on the host.  n1 >= 1,
// n2 >= 1, arguments checked by the caller.  tap (optional): forced split count, stage mask, and what the stages did.
static int fginn_search_and_walk(modsx_ctx *c, bool bytes, const void *d1, int n1, const void *d2, int n2, int dim, const double *pos2,
                                 double ratioT, double contradDist, int nn, std::vector<modsx_tentative> &out, const Fginn32Tap *tap, int dist) {
  out.clear();
  CtxBusy busy(c);
  const int stageMask = tap ? tap->stageMask : 3;
  const Fginn32Geo g = bytes ? fginn_l1_geometry(n1, n2, tap ? tap->splits : 0) : fginn32_geometry(n1, n2, dim, tap ? tap->splits : 0);
  if (tap && tap->geometry) geo_out(g, tap->geometry);
  const double rsq = ratioT * ratioT, cd2 = contradDist * contradDist;
  const size_t rowB = 16 + (size_t)n1 * 32;
  if (!c->matchWork.ensure(fginn32_workspace_bytes(g, n1)) || !c->matchRows.ensure(rowB) || !c->hMatch.ensure(rowB)) return MODSX_ERR_NOMEM;
  int rc = search_download(c, [&](hipEvent_t *ev) {      // timed under modsx_profile (tools/bench_fginn32.py)
    if (bytes) launch_fginn_l1_topk(c->stream, g, (const uint8_t *)d1, n1, (const uint8_t *)d2, n2, c->matchWork.p, c->matchRows.p, ev);
    else launch_fginn32_topk(c->stream, g, (const float *)d1, n1, (const float *)d2, n2, c->matchWork.p, c->matchRows.p, ev, dist);
  }, c->matchRows.p, c->hMatch.p, rowB, c->fginn32Ms);
  if (rc) return rc;
  const unsigned flag = *(const unsigned *)c->hMatch.p;
  if (tap && tap->counters) { tap->counters[0] = tap->counters[1] = tap->counters[2] = 0; tap->counters[3] = (int)flag; }
  if (flag) {
    set_error(std::string("modsx_match_fginn_f32: rows must be finite with |x| <= 1e17 (") + (flag & 1 ? "queries" : "") +
              (flag == 3 ? ", " : "") + (flag & 2 ? "trains" : "") + ")");
    return MODSX_ERR_ARG;
  }
  // the keys are copied: the stages below reuse hMatch
  std::vector<unsigned long long> top4((size_t)n1 * 4);
  memcpy(top4.data(), (const char *)c->hMatch.p + 16, (size_t)n1 * 32);
  if (tap && tap->top4) memcpy(tap->top4, top4.data(), (size_t)n1 * 32);

  FginnWalk walk;
  std::vector<F32Open> open;
  fginn_walk_open(top4.data(), n1, pos2, rsq, cd2, nn, 0, walk, open);

  // the open queries go through one more sweep: open[] and the initial closed[] up, closed[] down
  int nByCount = 0;
  if (!open.empty() && (stageMask & 2)) {
    const Fginn32Work w = fginn32_work(g, n1, c->matchWork.p);
    const int nu = (int)open.size();
    std::vector<F32Closed> closed;
    if (!c->pos2.ensure((size_t)n2 * 16)) return MODSX_ERR_NOMEM;
    MX_HIP(hipMemcpyAsync(c->pos2.p, pos2, (size_t)n2 * 16, hipMemcpyHostToDevice, c->stream));
    rc = resolve_round_trip(c, open, w.open, w.closed, closed, [&] {
      if (bytes) launch_fginn_l1_resolve(c->stream, g, n1, nu, n2, (const double *)c->pos2.p, cd2, c->matchWork.p);
      else launch_fginn32_resolve(c->stream, g, n1, nu, n2, (const double *)c->pos2.p, cd2, c->matchWork.p, dist);
    });
    if (rc) return rc;
    nByCount = fginn_walk_close(open, closed.data(), top4.data(), n1, rsq, nn, &walk);
  }
  fginn_walk_emit(walk, out);
  if (tap && tap->stage) memcpy(tap->stage, walk.stage.data(), n1);
  if (tap && tap->counters) { tap->counters[0] = (int)open.size(); tap->counters[1] = nByCount; tap->counters[2] = (int)out.size(); }
  return MODSX_OK;
}

int match_fginn32_device(modsx_ctx *c, const float *d1, int n1, const float *d2, int n2, int dim, const double *pos2, double ratioT,
                         double contradDist, int nn, std::vector<modsx_tentative> &out, const Fginn32Tap *tap, int dist) {
  return fginn_search_and_walk(c, false, d1, n1, d2, n2, dim, pos2, ratioT, contradDist, nn, out, tap, dist);
}
// the L1 search on dense [n][128] u8 rows in HBM (any alignment)
int match_fginn_l1_device(modsx_ctx *c, const uint8_t *d1, int n1, const uint8_t *d2, int n2, const double *pos2, double ratioT,
                          double contradDist, int nn, std::vector<modsx_tentative> &out, const Fginn32Tap *tap) {
  return fginn_search_and_walk(c, true, d1, n1, d2, n2, 128, pos2, ratioT, contradDist, nn, out, tap, MODSX_DIST_L1);
}

// rows from the host: checked here, uploaded, matched
int match_fginn32_host(modsx_ctx *c, const float *desc1, int n1, const float *desc2, int n2, int dim, const double *pos2, double ratioT,
                       double contradDist, int nn, std::vector<modsx_tentative> &out, const Fginn32Tap *tap, int dist) {
  out.clear();
  int rc = fginn32_check_args("modsx_match_fginn_f32", n1, n2, dim, ratioT, nn);
  if (rc) return rc;
  if ((rc = fginn32_check_dist("modsx_match_fginn_f32", dist))) return rc;
  if (n1 == 0 || n2 == 0) return MODSX_OK;
  const size_t f1 = (size_t)n1 * dim, f2 = (size_t)n2 * dim;
  if (!fginn32_rows_ok(desc1, f1) || !fginn32_rows_ok(desc2, f2)) {
    set_error("modsx_match_fginn_f32: rows must be finite with |x| <= 1e17");
    return MODSX_ERR_ARG;
  }
  CtxBusy busy(c);
  if ((rc = upload_row_pair(c, c->descF, desc1, f1 * 4, desc2, f2 * 4))) return rc;
  return match_fginn32_device(c, (const float *)c->descF[0].p, n1, (const float *)c->descF[1].p, n2, dim, pos2, ratioT, contradDist, nn, out, tap,
                              dist);
}

// [n][128] f32 rows from the host that hold the integers 0..255 (the domain of modsx_match_fginn): narrowed to bytes, uploaded, matched
int match_fginn_l1_host(modsx_ctx *c, const float *desc1, int n1, const float *desc2, int n2, const double *pos2, double ratioT,
                        double contradDist, int nn, std::vector<modsx_tentative> &out, const Fginn32Tap *tap) {
  out.clear();
  int rc = fginn32_check_args("modsx_match_fginn_l1", n1, n2, 128, ratioT, nn);
  if (rc) return rc;
  if (n1 == 0 || n2 == 0) return MODSX_OK;
  std::vector<uint8_t> u1((size_t)n1 * 128), u2((size_t)n2 * 128);
  if (!desc_f32_to_u8(desc1, u1.size(), u1.data()) || !desc_f32_to_u8(desc2, u2.size(), u2.data())) {
    set_error("modsx_match_fginn_l1: descriptors must hold the integers 0..255 (SIFT-family quantisation)");
    return MODSX_ERR_ARG;
  }
  CtxBusy busy(c);
  if ((rc = upload_row_pair(c, c->descU8, u1.data(), u1.size(), u2.data(), u2.size()))) return rc;
  return match_fginn_l1_device(c, (const uint8_t *)c->descU8[0].p, n1, (const uint8_t *)c->descU8[1].p, n2, pos2, ratioT, contradDist, nn, out, tap);
}

// MatchFlannFGINN + DuplicateFiltering + LORANSACFiltering on caller-supplied regions: what match_pair leaves with the match stage
// replaced.  pos2 = reproj_kp of the second list, as the reference takes it.  An empty side gives the zeroed result with H = -1.
// bytes: the rows hold the integers 0..255 at dim = 128 and go through the L1 search on bytes (dist is then L1)
int match_regions_f32(modsx_ctx *c, const modsx_region *regs1, const float *desc1, int n1, const modsx_region *regs2, const float *desc2,
                      int n2, int dim, const modsx_pair_params &pp, modsx_pair_result *res, int dist, bool bytes) {
  return match_regions_with(regs1, n1, regs2, n2, pp, res, [&](std::vector<modsx_tentative> &tents) {
    const char *fn = bytes ? "modsx_match_regions_l1" : "modsx_match_regions_f32";
    int rc = fginn32_check_args(fn, n1, n2, dim, pp.match_ratio, pp.nn);
    if (rc) return rc;
    if ((rc = fginn32_check_dist(fn, dist))) return rc;
    std::vector<double> pos2((size_t)n2 * 2);
    for (int i = 0; i < n2; i++) { pos2[2 * (size_t)i] = regs2[i].reproj_kp.x; pos2[2 * (size_t)i + 1] = regs2[i].reproj_kp.y; }
    return bytes ? match_fginn_l1_host(c, desc1, n1, desc2, n2, pos2.data(), pp.match_ratio, pp.contradDist, pp.nn, tents, nullptr)
                 : match_fginn32_host(c, desc1, n1, desc2, n2, dim, pos2.data(), pp.match_ratio, pp.contradDist, pp.nn, tents, nullptr, dist);
  });
}

}  // namespace mx
