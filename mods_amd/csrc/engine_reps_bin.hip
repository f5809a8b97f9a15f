// engine_reps_bin.hip -- the binary descriptor classes of a stored image representation (ORB, BRISK, FREAK).
//
//   ImageRepresentation::RegionVectorMap[det][desc]      any descriptor name                       (one RepSlotB per class)
//   LoadRegions                                          imagerepresentation.cpp:2139-2215         (rep_append_bin)
//   MatchImgReps: MatchFLANNDistance on a binary class   correspondencebank.cpp:291-347            (reps_bin_match_group)
// A slot keeps its rows exactly as k_hamming_pack writes them (kernels_hamming.hip: WK dwords per row, zero behind nbytes) with
// zero rows up to its capacity, a multiple of 1024 rows: whole workgroups of queries and whole tiles of trains at every WK.  Nothing
// is packed when a slot is matched, and an append only packs behind the old rows.  The store itself (release, reserve, the
// zero-again rollback, the class download) is the one the float slots use too and lives in engine_reps.hip with the class table;
// here are the pack kernel, the width rule and the search.  The search is the grouped launch set of
// kernels_hamming.hip; it has no walk and no resolve pass, so a group of partners costs one search launch, one merge launch and
// ONE host round trip, where matching its partners one by one costs two pack launches, two search launches and a round trip each.
// The record rule is the one copy in engine_hamming.hip (hamming_tentatives), applied per partner.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "engine_api.hpp"

namespace mx {

static RepSlotB &bslot(modsx_rep *rep, int det, int type) { return rep->bslot[det][type - MODSX_DESC_BRISK]; }
static const RepSlotB &bslot(const modsx_rep *rep, int det, int type) { return rep->bslot[det][type - MODSX_DESC_BRISK]; }

// dense: [n][nbytes] u8 in HBM, any alignment.  The rows are packed behind the old ones; the count moves only when that is done
static int slot_store(modsx_ctx *c, RepSlotB &k, int nbytes, const modsx_region *regs, const uint8_t *dense, int n) {
  const int WK = hamming_kernel_width((nbytes + 3) / 4);
  const size_t base = k.regs.size();
  const int rc = slot_reserve(c, k, base + (size_t)n, WK, false);
  if (rc) return rc;
  launch_hamming_pack_rows(c->stream, dense, n, nbytes, WK, (uint32_t *)k.rows.p + base * WK);
  hipError_t e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) {                                    // the padding behind the old rows is zero again, if the device still answers
    slot_zero_again(c, k, base, n);
    MX_HIP(e);
  }
  k.nbytes = nbytes; k.W = WK;
  k.regs.insert(k.regs.end(), regs, regs + n);
  c->hamGroupCounters[2] += n;
  return MODSX_OK;
}

// rows: [n][nbytes] u8, on the host or (onDevice) in HBM
int rep_append_bin(modsx_ctx *c, modsx_rep *rep, int det, int type, const modsx_region *regs, const uint8_t *rows, bool onDevice,
                   int nbytes, int n, const char *fn) {
  CtxBusy busy(c);
  const std::string f(fn);
  RepSlotB &k = bslot(rep, det, type);
  if (rep->dev != c->dev) { set_error(f + ": the representation lives on another device"); return MODSX_ERR_ARG; }
  if (nbytes < 1 || nbytes > MODSX_HAMMING_MAX_BYTES) { set_error(f + ": nbytes must be in [1, MODSX_HAMMING_MAX_BYTES]"); return MODSX_ERR_ARG; }
  if (k.nbytes && k.nbytes != nbytes) { set_error(f + ": the class holds rows of another width"); return MODSX_ERR_ARG; }
  if (k.regs.size() + (size_t)n > 2000000) { set_error(f + ": more than 2 000 000 regions in one class"); return MODSX_ERR_ARG; }
  if (n == 0) return 0;
  int rc = MODSX_OK;
  if (!onDevice) {
    const size_t bytes = (size_t)n * nbytes;
    if (!c->repStage.ensure(bytes)) rc = MODSX_ERR_NOMEM;
    if (!rc) {
      hipError_t e = hipMemcpyAsync(c->repStage.p, rows, bytes, hipMemcpyHostToDevice, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);      // the source is pageable and may be the caller's temporary
      if (e != hipSuccess) { set_error(f + ": " + hipGetErrorString(e)); rc = MODSX_ERR_DEVICE; }
    }
    rows = (const uint8_t *)c->repStage.p;
  }
  if (!rc) rc = slot_store(c, k, nbytes, regs, rows, n);
  if (rc && k.regs.empty()) slot_release(k);               // a class that is still empty has no width yet, so it keeps no buffer
  return rc ? rc : n;
}

int rep_class_bin(modsx_ctx *c, const modsx_rep *rep, int det, int type, modsx_region **regs, unsigned char **rows, int *nbytes) {
  const RepSlotB &k = bslot(rep, det, type);
  if (nbytes) *nbytes = k.regs.empty() ? 0 : k.nbytes;
  return slot_download(c, "modsx_rep_class_bin", k, (size_t)k.nbytes, regs, (void **)rows);      // a packed row is its bytes in order
}

int reps_bin_check(const char *fn, const modsx_ctx *c, const modsx_rep *rep1, const modsx_rep *const *reps2, int n, int det, int type,
                   double distanceThreshold) {
  const std::string f(fn);
  const RepSlotB &q = bslot(rep1, det, type);
  int nbytes = q.regs.empty() ? 0 : q.nbytes;
  if (rep1->dev != c->dev) { set_error(f + ": a representation lives on another device"); return MODSX_ERR_ARG; }
  for (int g = 0; g < n; g++) {
    if (reps2[g]->dev != c->dev) { set_error(f + ": a representation lives on another device"); return MODSX_ERR_ARG; }
    const RepSlotB &t = bslot(reps2[g], det, type);
    if (t.regs.empty()) continue;
    if (!nbytes) nbytes = t.nbytes;
    if (t.nbytes != nbytes) { set_error(f + ": the class has different widths in the two representations"); return MODSX_ERR_ARG; }
    const int rc = hamming_check_args(fn, (int)q.regs.size(), (int)t.regs.size(), nbytes);      // a train class of one region
    if (rc) return rc;
  }
  std::vector<modsx_tentative> none;
  return hamming_tentatives(nullptr, 0, distanceThreshold, none);      // the threshold's refusal lives with the record rule
}

int reps_bin_match_group(modsx_ctx *c, const char *fn, const modsx_rep *rep1, const modsx_rep *const *reps2, int G, int det, int type,
                         double distanceThreshold, std::vector<modsx_tentative> *outs) {
  if (G < 1 || G > MATCH_MAXB) { set_error(std::string(fn) + ": a group holds 1 .. 4 partners"); return MODSX_ERR_ARG; }
  for (int g = 0; g < G; g++) outs[g].clear();
  int rc = reps_bin_check(fn, c, rep1, reps2, G, det, type, distanceThreshold);
  if (rc) return rc;
  const RepSlotB &q = bslot(rep1, det, type);
  const int n1 = (int)q.regs.size();
  int n2[MATCH_MAXB];
  for (int g = 0; g < G; g++) n2[g] = (int)bslot(reps2[g], det, type).regs.size();
  HamGroup grp;
  int prob[MATCH_MAXB];
  if (n1 == 0 || hamming_group_geometry(n1, n2, G, (q.nbytes + 3) / 4, grp, prob) == 0) return MODSX_OK;
  for (int p = 0; p < grp.np; p++) grp.trains[p] = (const uint32_t *)bslot(reps2[prob[p]], det, type).rows.p;

  CtxBusy busy(c);
  const int np = grp.np;
  // workspace: the split keys [splits][n1][2]; the merged results [np][n1][4] travel through matchRows
  const size_t keyB = (size_t)grp.first[np] * n1 * 16, outB = (size_t)np * n1 * 16;
  if (!c->matchWork.ensure(keyB) || !c->matchRows.ensure(outB) || !c->hMatch.ensure(outB)) return MODSX_ERR_NOMEM;
  rc = search_download(c, [&](hipEvent_t *) {
    launch_hamming_group(c->stream, grp, (const uint32_t *)q.rows.p, n1, (unsigned long long *)c->matchWork.p, (int *)c->matchRows.p);
  }, c->matchRows.p, c->hMatch.p, outB, nullptr);
  if (rc) return rc;
  c->hamGroupCounters[0]++; c->hamGroupCounters[1] += np;
  const int *nn2 = (const int *)c->hMatch.p;
  for (int p = 0; p < np && !rc; p++) rc = hamming_tentatives(nn2 + (size_t)p * n1 * 4, n1, distanceThreshold, outs[prob[p]]);
  return rc;
}

}  // namespace mx

using namespace mx;

extern "C" {

int modsx_rep_append_bin(modsx_ctx *ctx, modsx_rep *rep, int detector, int desc_type, const modsx_region *regs, const void *desc,
                         int nbytes, int dtype, int n) {
  const char *fn = "modsx_rep_append_bin";
  int det;
  if (!ctx || !rep || n < 0 || (n > 0 && (!regs || !desc)) || !rep_class_bin_ok(detector, desc_type, &det)) {
    set_error("modsx_rep_append_bin: bad argument (detector HessianAffine / MSER / ORB / SURF, descriptor type MODSX_DESC_BRISK .. MODSX_DESC_ORB, n >= 0 regions with [n][nbytes] rows)");
    return MODSX_ERR_ARG;
  }
  if (dtype != 0 && dtype != 1) { set_error("modsx_rep_append_bin: dtype must be 0 (u8) or 1 (f32)"); return MODSX_ERR_ARG; }
  if (nbytes < 1 || nbytes > MODSX_HAMMING_MAX_BYTES) { set_error("modsx_rep_append_bin: nbytes must be in [1, MODSX_HAMMING_MAX_BYTES]"); return MODSX_ERR_ARG; }
  std::vector<uint8_t> conv;
  const uint8_t *u8 = (const uint8_t *)desc;
  if (dtype == 1 && n > 0) {
    conv.resize((size_t)n * nbytes);
    if (!desc_f32_to_u8((const float *)desc, conv.size(), conv.data())) {
      set_error("modsx_rep_append_bin: f32 descriptors must hold the integers 0..255");
      return MODSX_ERR_ARG;
    }
    u8 = conv.data();
  }
  hipSetDevice(ctx->dev);
  return rep_append_bin(ctx, rep, det, desc_type, regs, u8, false, nbytes, n, fn);
}

int modsx_rep_append_bin_device(modsx_ctx *ctx, modsx_rep *rep, int detector, int desc_type, const modsx_region *regs,
                                const void *dev_desc_u8, int nbytes, int n) {
  int det;
  if (!ctx || !rep || n < 0 || (n > 0 && (!regs || !dev_desc_u8)) || !rep_class_bin_ok(detector, desc_type, &det)) {
    set_error("modsx_rep_append_bin_device: bad argument (detector HessianAffine / MSER / ORB / SURF, descriptor type MODSX_DESC_BRISK .. MODSX_DESC_ORB, n >= 0 regions with [n][nbytes] rows)");
    return MODSX_ERR_ARG;
  }
  hipSetDevice(ctx->dev);
  return rep_append_bin(ctx, rep, det, desc_type, regs, (const uint8_t *)dev_desc_u8, true, nbytes, n, "modsx_rep_append_bin_device");
}

int modsx_rep_class_bin(modsx_ctx *ctx, const modsx_rep *rep, int detector, int desc_type, modsx_region **regs, unsigned char **desc_u8,
                        int *nbytes) {
  int det;
  if (!ctx || !rep || !rep_class_bin_ok(detector, desc_type, &det)) { set_error("modsx_rep_class_bin: bad argument"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  return rep_class_bin(ctx, rep, det, desc_type, regs, desc_u8, nbytes);
}

int modsx_rep_match_group_hamming(modsx_ctx *ctx, const modsx_rep *rep1, const modsx_rep *const *reps2, int G, int detector,
                                  int desc_type, double distanceThreshold, modsx_tentative **outs, int *counts) {
  int det;
  bool ok = ctx && rep1 && reps2 && outs && counts && G >= 1 && G <= MATCH_MAXB && rep_class_bin_ok(detector, desc_type, &det);
  for (int g = 0; ok && g < G; g++) ok = reps2[g] != nullptr;
  if (!ok) { set_error("modsx_rep_match_group_hamming: bad argument (1 .. 4 partners, a binary class)"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  std::vector<modsx_tentative> t[MATCH_MAXB];
  const int rc = reps_bin_match_group(ctx, "modsx_rep_match_group_hamming", rep1, reps2, G, det, desc_type, distanceThreshold, t);
  if (rc) return rc;
  for (int g = 0; g < G; g++) { outs[g] = to_malloc(t[g]); counts[g] = (int)t[g].size(); }
  return G;
}

int modsx_rep_match_hamming(modsx_ctx *ctx, const modsx_rep *rep1, const modsx_rep *rep2, int detector, int desc_type,
                            double distanceThreshold, modsx_tentative **out) {
  int det;
  if (!ctx || !rep1 || !rep2 || !out || !rep_class_bin_ok(detector, desc_type, &det)) { set_error("modsx_rep_match_hamming: bad argument"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  std::vector<modsx_tentative> t;
  const int rc = reps_bin_match_group(ctx, "modsx_rep_match_hamming", rep1, &rep2, 1, det, desc_type, distanceThreshold, &t);
  if (rc) return rc;
  *out = to_malloc(t);
  return (int)t.size();
}

int modsx_debug_hamming_group_geometry(int n1, const int *n2, int G, int nbytes, int *geometry, int *per_problem, int *splits, int cap) {
  if (!n2 || !geometry || !per_problem || G < 1 || G > MATCH_MAXB || n1 < 1 || cap < 0 || (cap > 0 && !splits)) {
    set_error("modsx_debug_hamming_group_geometry: bad argument (n1 >= 1, 1 .. 4 partners)");
    return MODSX_ERR_ARG;
  }
  for (int g = 0; g < G; g++) {
    const int rc = hamming_check_args("modsx_debug_hamming_group_geometry", n1, n2[g], nbytes);
    if (rc) return rc;
  }
  HamGroup g;
  int prob[MATCH_MAXB];
  const int total = hamming_group_geometry(n1, n2, G, (nbytes + 3) / 4, g, prob);
  return group_geometry_report(g, g.WK, prob, G, total, geometry, per_problem, splits, cap);
}

int modsx_hamming_group_counters(modsx_ctx *ctx, long *out, int n) {
  if (!ctx || n < 0 || (n > 0 && !out)) { set_error("modsx_hamming_group_counters: bad argument"); return MODSX_ERR_ARG; }
  for (int i = 0; i < n && i < 4; i++) out[i] = ctx->hamGroupCounters[i];
  return 4;
}

}  // extern "C"
