// engine_reps_f32.hip -- the float descriptor classes of a stored image representation (SURF, LIOP, DAISY, MROGH, learned vectors).
//
//   ImageRepresentation::RegionVectorMap[det][desc]      any descriptor name                       (one RepSlotF per class)
//   LoadRegions                                          imagerepresentation.cpp:2139-2215         (rep_append_f32)
//   DescribeRegions<SURF / LIOP / DAISY>                 imagerepresentation.cpp:1829-1838, 1954-1963   (rep_describe_append)
//   MatchImgReps: MatchFlannFGINN on every class         correspondencebank.cpp:291-347            (reps_f32_match_group)
// A slot keeps its rows in the row form of the f32 matcher (kernels_fginn32.hip: DK floats per row, zero behind dim) with zero rows
// up to its capacity, a multiple of 256: whole workgroups of queries and whole tiles of trains at every tile length.  Nothing is
// packed when a slot is matched, and an append only writes behind the old rows.  The store itself (release, reserve, the zero-again
// rollback, the class download) is the one the binary slots use too and lives in engine_reps.hip with the class table; here are
// the pack kernel, the flag word, the host positions and the width rules.  The search is the grouped launch set of
// kernels_fginn32.hip; the walk over the four nearest neighbours is fginn_walk.hpp, the one the single call runs, opened per
// problem on the one copy of all problems' keys; the walks left open in any problem share one resolve launch and one close step.
// So a group costs two host round trips, where matching its partners one by one costs two each and packs both sides every time.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "engine_api.hpp"

namespace mx {

static RepSlotF &fslot(modsx_rep *rep, int det, int type) { return rep->fslot[det][type - MODSX_DESC_CAFFE]; }
static const RepSlotF &fslot(const modsx_rep *rep, int det, int type) { return rep->fslot[det][type - MODSX_DESC_CAFFE]; }

// the widths a type takes
static bool width_fits(int type, int dim) {
  if (dim < 4 || dim > MODSX_FGINN32_MAX_DIM || dim % 4) return false;
  switch (type) {
    case MODSX_DESC_SURF: return dim == 64;
    case MODSX_DESC_LIOP: return dim == 144;
    case MODSX_DESC_MROGH: return dim == 192;
    case MODSX_DESC_DAISY:
      for (int radq = 1; radq <= 3; radq++) for (int thq = 1; thq <= 8; thq++) if ((radq * thq + 1) * 8 == dim) return true;
      return false;
    default: return true;
  }
}

// what every append checks before it touches the slot
static int append_args(const char *fn, modsx_ctx *c, const modsx_rep *rep, const RepSlotF &k, int type, int dim, int n) {
  const std::string f(fn);
  if (rep->dev != c->dev) { set_error(f + ": the representation lives on another device"); return MODSX_ERR_ARG; }
  if (!width_fits(type, dim)) { set_error(f + ": the descriptor type does not have this width"); return MODSX_ERR_ARG; }
  if (k.dim && k.dim != dim) { set_error(f + ": the class holds rows of another width"); return MODSX_ERR_ARG; }
  if (k.regs.size() + (size_t)n > 2000000) { set_error(f + ": more than 2 000 000 regions in one class"); return MODSX_ERR_ARG; }
  return MODSX_OK;
}

// dense: [n][dim] f32 in HBM.  The rows enter the slot behind the old ones through the matcher's pack kernel, which also holds the
// validity check; a row it flags takes the new rows out again (back to zero rows) and the slot is what it was.  A class that is
// still empty when an append fails, for whatever reason, gives its buffers back: it has no width yet, so it keeps none.
static int slot_store(const char *fn, modsx_ctx *c, RepSlotF &k, int dim, const modsx_region *regs, const float *dense, int n);
static int slot_ingest(const char *fn, modsx_ctx *c, RepSlotF &k, int dim, const modsx_region *regs, const float *dense, int n) {
  const int rc = slot_store(fn, c, k, dim, regs, dense, n);
  if (rc && k.regs.empty()) slot_release(k);
  return rc;
}
static int slot_store(const char *fn, modsx_ctx *c, RepSlotF &k, int dim, const modsx_region *regs, const float *dense, int n) {
  const int DK = fginn32_kernel_width(dim);
  const size_t base = k.regs.size();
  int rc = slot_reserve(c, k, base + (size_t)n, DK, true);
  if (rc) return rc;
  if (!c->matchRows.ensure(16)) return MODSX_ERR_NOMEM;
  unsigned *flag = (unsigned *)c->matchRows.p, hflag = 0;
  float *dst = (float *)k.rows.p + base * DK;
  std::vector<double> pos((size_t)n * 2);
  for (int i = 0; i < n; i++) { pos[2 * (size_t)i] = regs[i].reproj_kp.x; pos[2 * (size_t)i + 1] = regs[i].reproj_kp.y; }
  MX_HIP(hipMemsetAsync(flag, 0, 16, c->stream));
  launch_fginn32_pack_rows(c->stream, dense, n, dim, DK, dst, flag, 1u);
  MX_HIP(hipMemcpyAsync((double *)k.pos.p + base * 2, pos.data(), (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
  MX_HIP(hipMemcpyAsync(&hflag, flag, 4, hipMemcpyDeviceToHost, c->stream));
  MX_HIP(hipStreamSynchronize(c->stream));
  MX_HIP(hipGetLastError());
  if (hflag) {
    MX_HIP(slot_zero_again(c, k, base, n));
    set_error(std::string(fn) + ": rows must be finite with |x| <= 1e17");
    return MODSX_ERR_ARG;
  }
  k.dim = dim; k.W = DK;
  k.regs.insert(k.regs.end(), regs, regs + n);
  k.hpos.insert(k.hpos.end(), pos.begin(), pos.end());
  return MODSX_OK;
}

int rep_append_f32(modsx_ctx *c, modsx_rep *rep, int det, int type, const modsx_region *regs, const float *rows, int dim, int n,
                   bool onDevice) {
  CtxBusy busy(c);
  RepSlotF &k = fslot(rep, det, type);
  int rc = append_args(onDevice ? "modsx_rep_append_f32_device" : "modsx_rep_append_f32", c, rep, k, type, dim, n);
  if (rc) return rc;
  if (n == 0) return 0;
  if (onDevice) {      // the rows are read where they lie; the pack kernel's flag word is the validity check
    rc = slot_ingest("modsx_rep_append_f32_device", c, k, dim, regs, rows, n);
    return rc ? rc : n;
  }
  const size_t floats = (size_t)n * dim;
  if (!fginn32_rows_ok(rows, floats)) { set_error("modsx_rep_append_f32: rows must be finite with |x| <= 1e17"); return MODSX_ERR_ARG; }
  if (!c->repStage.ensure(floats * 4)) return MODSX_ERR_NOMEM;
  MX_HIP(hipMemcpyAsync(c->repStage.p, rows, floats * 4, hipMemcpyHostToDevice, c->stream));
  rc = slot_ingest("modsx_rep_append_f32", c, k, dim, regs, (const float *)c->repStage.p, n);
  return rc ? rc : n;
}

int rep_describe_append(modsx_ctx *c, modsx_rep *rep, int det, int type, const modsx_image *img, const modsx_region *regs, int n,
                        double mrSize, int patchSize, int fast, int photoNorm, const int *dp) {
  const char *fn = "modsx_rep_describe_append";
  int dim = 0, rc = MODSX_OK;
  switch (type) {
    case MODSX_DESC_SURF: dim = 64; rc = surf_check_args(fn, patchSize, mrSize); break;
    case MODSX_DESC_LIOP:
      dim = 144;
      if (patchSize != 41) { set_error(std::string(fn) + ": patchSize must be 41"); rc = MODSX_ERR_ARG; }
      break;
    case MODSX_DESC_DAISY:
      if (!dp) { set_error(std::string(fn) + ": DAISY needs daisy_par = {rad, radq, thq, histq, nrm_type}"); return MODSX_ERR_ARG; }
      rc = daisy_check_args(fn, patchSize, dp[0], dp[1], dp[2], dp[3], dp[4]);
      if (!rc) dim = daisy_dim(dp[1], dp[2], dp[3]);
      break;
    default:
      set_error(std::string(fn) + ": the type has no extractor here (SURF, LIOP and DAISY have; CAFFE and MROGH rows come from the caller)");
      return MODSX_ERR_ARG;
  }
  if (rc) return rc;
  CtxBusy busy(c);
  RepSlotF &k = fslot(rep, det, type);
  if ((rc = append_args(fn, c, rep, k, type, dim, n))) return rc;
  if (n == 0) return 0;
  // the extractor's dense rows stay on the device: its kernels write repStage, the pack kernel reads it
  if (!c->repStage.ensure((size_t)n * dim * 4)) return MODSX_ERR_NOMEM;
  float *dense = (float *)c->repStage.p;
  if (type == MODSX_DESC_SURF) rc = describe_regions_surf(c, img, regs, n, mrSize, patchSize, fast, photoNorm, dense, true);
  else if (type == MODSX_DESC_LIOP) rc = describe_regions_liop(c, img, regs, n, mrSize, patchSize, fast, photoNorm, dense, true);
  else rc = describe_regions_daisy(c, img, regs, n, mrSize, patchSize, fast, photoNorm, dp[0], dp[1], dp[2], dp[4], dense, true);
  if (rc) return rc;
  rc = slot_ingest(fn, c, k, dim, regs, dense, n);
  return rc ? rc : n;
}

int rep_class_f32(modsx_ctx *c, const modsx_rep *rep, int det, int type, modsx_region **regs, float **rows, int *dim) {
  const RepSlotF &k = fslot(rep, det, type);
  if (dim) *dim = k.dim;
  return slot_download(c, "modsx_rep_class_f32", k, (size_t)k.dim * 4, regs, (void **)rows);
}

int reps_f32_match_group(modsx_ctx *c, const char *fn, const modsx_rep *rep1, const modsx_rep *const *reps2, int G, int det, int type,
                         double ratioT, double contradDist, int nn, std::vector<modsx_tentative> *outs) {
  const std::string f(fn);
  if (G < 1 || G > MATCH_MAXB) { set_error(f + ": a group holds 1 .. 4 partners"); return MODSX_ERR_ARG; }
  for (int g = 0; g < G; g++) outs[g].clear();
  const RepSlotF &q = fslot(rep1, det, type);
  const RepSlotF *t[MATCH_MAXB];
  int n2[MATCH_MAXB], dim = q.dim;
  const int n1 = (int)q.regs.size();
  for (int g = 0; g < G; g++) {
    if (rep1->dev != c->dev || reps2[g]->dev != c->dev) { set_error(f + ": a representation lives on another device"); return MODSX_ERR_ARG; }
    t[g] = &fslot(reps2[g], det, type);
    n2[g] = (int)t[g]->regs.size();
    if (!dim) dim = t[g]->dim;
    if (t[g]->dim && t[g]->dim != dim) { set_error(f + ": the class has different widths in the two representations"); return MODSX_ERR_ARG; }
  }
  int rc = fginn32_check_args(fn, n1, *std::max_element(n2, n2 + G), dim ? dim : 4, ratioT, nn);
  if (rc) return rc;
  F32Group grp;
  int prob[MATCH_MAXB];
  if (n1 == 0 || fginn32_group_geometry(n1, n2, G, dim, grp, prob) == 0) return MODSX_OK;
  for (int p = 0; p < grp.np; p++) { grp.trains[p] = (const float *)t[prob[p]]->rows.p; grp.pos[p] = (const double *)t[prob[p]]->pos.p; }

  CtxBusy busy(c);
  const double rsq = ratioT * ratioT, cd2 = contradDist * contradDist;
  const int np = grp.np, splits = grp.first[np];
  // workspace: split keys [splits][n1][4] | open [np * n1] | closed [np * n1]; the merged keys [np][n1][4] travel through matchRows
  const size_t keyB = (size_t)splits * n1 * 32, topB = (size_t)np * n1 * 32, openB = align_up((size_t)np * n1 * sizeof(F32Open), 256);
  if (!c->matchWork.ensure(keyB + openB + (size_t)np * n1 * sizeof(F32Closed)) || !c->matchRows.ensure(topB) || !c->hMatch.ensure(topB))
    return MODSX_ERR_NOMEM;
  unsigned long long *keys = (unsigned long long *)c->matchWork.p;
  F32Open *dOpen = (F32Open *)((char *)c->matchWork.p + keyB);
  F32Closed *dClosed = (F32Closed *)((char *)dOpen + openB);
  rc = search_download(c, [&](hipEvent_t *) {
    launch_fginn32_group_topk(c->stream, grp, (const float *)q.rows.p, n1, keys, (unsigned long long *)c->matchRows.p);
  }, c->matchRows.p, c->hMatch.p, topB, nullptr);
  if (rc) return rc;
  c->f32GroupCounters[0]++; c->f32GroupCounters[1] += np;
  // The keys are read where the copy left them (pinned host memory; nothing below writes there): the walk of fginn_walk.hpp, one
  // open step per problem, all problems' open entries in one list
  const unsigned long long *top4 = (const unsigned long long *)c->hMatch.p;
  FginnWalk walks[MATCH_MAXB];
  std::vector<F32Open> open;
  for (int p = 0; p < np; p++) {
    grp.ubeg[p] = (int)open.size();
    fginn_walk_open(top4 + (size_t)p * n1 * 4, n1, t[prob[p]]->hpos.data(), rsq, cd2, nn, p, walks[p], open);
    grp.uend[p] = (int)open.size();
  }

  // every open walk of every problem goes through one more sweep, in one launch
  if (!open.empty()) {
    const int nu = (int)open.size();
    int rfirst = 0;
    for (int p = 0; p < np; p++) { grp.rfirst[p] = rfirst; rfirst += (grp.uend[p] - grp.ubeg[p] + 255) / 256 * grp.S[p]; }
    for (int p = np; p <= MATCH_MAXB; p++) grp.rfirst[p] = rfirst;
    std::vector<F32Closed> closed;
    rc = resolve_round_trip(c, open, dOpen, dClosed, closed,
                            [&] { launch_fginn32_group_resolve(c->stream, grp, (const float *)q.rows.p, dOpen, cd2, dClosed); });
    if (rc) return rc;
    c->f32GroupCounters[2] += nu; c->f32GroupCounters[3]++;
    fginn_walk_close(open, closed.data(), top4, n1, rsq, nn, walks);
  }
  for (int p = 0; p < np; p++) fginn_walk_emit(walks[p], outs[prob[p]]);
  return MODSX_OK;
}

}  // namespace mx

using namespace mx;

extern "C" {

int modsx_rep_append_f32(modsx_ctx *ctx, modsx_rep *rep, int detector, int desc_type, const modsx_region *regs, const float *rows, int dim,
                         int n) {
  int det;
  if (!ctx || !rep || n < 0 || (n > 0 && (!regs || !rows)) || !rep_class_f32_ok(detector, desc_type, &det)) {
    set_error("modsx_rep_append_f32: bad argument (detector HessianAffine / MSER / SURF, descriptor type MODSX_DESC_CAFFE .. MODSX_DESC_SURF, n >= 0 regions with [n][dim] rows)");
    return MODSX_ERR_ARG;
  }
  hipSetDevice(ctx->dev);
  return rep_append_f32(ctx, rep, det, desc_type, regs, rows, dim, n);
}

int modsx_rep_append_f32_device(modsx_ctx *ctx, modsx_rep *rep, int detector, int desc_type, const modsx_region *regs, const void *dev_rows,
                                int dim, int n) {
  int det;
  if (!ctx || !rep || n < 0 || (n > 0 && (!regs || !dev_rows)) || ((uintptr_t)dev_rows & 3) || !rep_class_f32_ok(detector, desc_type, &det)) {
    set_error("modsx_rep_append_f32_device: bad argument (detector HessianAffine / MSER / SURF, descriptor type MODSX_DESC_CAFFE .. MODSX_DESC_SURF, n >= 0 regions with 4-byte aligned [n][dim] device rows)");
    return MODSX_ERR_ARG;
  }
  hipSetDevice(ctx->dev);
  return rep_append_f32(ctx, rep, det, desc_type, regs, (const float *)dev_rows, dim, n, true);
}

int modsx_rep_describe_append(modsx_ctx *ctx, modsx_rep *rep, int detector, int desc_type, const modsx_image *img, const modsx_region *regs,
                              int n, double mrSize, int patchSize, int fast_extraction, int photoNorm, const int *daisy_par) {
  int det;
  if (!ctx || !rep || !img || n < 0 || (n > 0 && !regs) || !rep_class_f32_ok(detector, desc_type, &det)) {
    set_error("modsx_rep_describe_append: bad argument (detector HessianAffine / MSER / SURF, a float descriptor type, an image, n >= 0 regions)");
    return MODSX_ERR_ARG;
  }
  hipSetDevice(ctx->dev);
  return rep_describe_append(ctx, rep, det, desc_type, img, regs, n, mrSize, patchSize, fast_extraction, photoNorm, daisy_par);
}

int modsx_rep_class_f32(modsx_ctx *ctx, const modsx_rep *rep, int detector, int desc_type, modsx_region **regs, float **rows, int *dim) {
  int det;
  if (!ctx || !rep || !rep_class_f32_ok(detector, desc_type, &det)) { set_error("modsx_rep_class_f32: bad argument"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  return rep_class_f32(ctx, rep, det, desc_type, regs, rows, dim);
}

int modsx_rep_match_group_f32(modsx_ctx *ctx, const modsx_rep *rep1, const modsx_rep *const *reps2, int G, int detector, int desc_type,
                              double ratio, double contradDist, int nn, modsx_tentative **outs, int *counts) {
  int det;
  bool ok = ctx && rep1 && reps2 && outs && counts && G >= 1 && G <= MATCH_MAXB && rep_class_f32_ok(detector, desc_type, &det);
  for (int g = 0; ok && g < G; g++) ok = reps2[g] != nullptr;
  if (!ok) { set_error("modsx_rep_match_group_f32: bad argument (1 .. 4 partners, a float class)"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  std::vector<modsx_tentative> t[MATCH_MAXB];
  const int rc = reps_f32_match_group(ctx, "modsx_rep_match_group_f32", rep1, reps2, G, det, desc_type, ratio, contradDist, nn, t);
  if (rc) return rc;
  for (int g = 0; g < G; g++) { outs[g] = to_malloc(t[g]); counts[g] = (int)t[g].size(); }
  return G;
}

int modsx_rep_match_fginn_f32(modsx_ctx *ctx, const modsx_rep *rep1, const modsx_rep *rep2, int detector, int desc_type, double ratio,
                              double contradDist, int nn, modsx_tentative **out) {
  int det;
  if (!ctx || !rep1 || !rep2 || !out || !rep_class_f32_ok(detector, desc_type, &det)) { set_error("modsx_rep_match_fginn_f32: bad argument"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  std::vector<modsx_tentative> t;
  const int rc = reps_f32_match_group(ctx, "modsx_rep_match_fginn_f32", rep1, &rep2, 1, det, desc_type, ratio, contradDist, nn, &t);
  if (rc) return rc;
  *out = to_malloc(t);
  return (int)t.size();
}

int modsx_debug_fginn32_group_geometry(int n1, const int *n2, int G, int dim, int *geometry, int *per_problem, int *splits, int cap) {
  if (!n2 || !geometry || !per_problem || G < 1 || G > MATCH_MAXB || n1 < 1 || cap < 0 || (cap > 0 && !splits)) {
    set_error("modsx_debug_fginn32_group_geometry: bad argument (n1 >= 1, 1 .. 4 partners)");
    return MODSX_ERR_ARG;
  }
  const int rc = fginn32_check_args("modsx_debug_fginn32_group_geometry", n1, *std::max_element(n2, n2 + G), dim, 0.5, 2);
  if (rc) return rc;
  F32Group g;
  int prob[MATCH_MAXB];
  const int total = fginn32_group_geometry(n1, n2, G, dim, g, prob);
  return group_geometry_report(g, g.DK, prob, G, total, geometry, per_problem, splits, cap);
}

int modsx_fginn32_group_counters(modsx_ctx *ctx, long *out, int n) {
  if (!ctx || n < 0 || (n > 0 && !out)) { set_error("modsx_fginn32_group_counters: bad argument"); return MODSX_ERR_ARG; }
  for (int i = 0; i < n && i < 4; i++) out[i] = ctx->f32GroupCounters[i];
  return 4;
}

}  // extern "C"
