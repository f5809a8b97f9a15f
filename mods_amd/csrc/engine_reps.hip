// engine_reps.hip -- stored image representations: describe an image once, match it against many.
//
//   ImageRepresentation::RegionVectorMap[det][desc]      imagerepresentation.hpp / .cpp:552-600   (one slot per class)
//   SynthDetectDescribeKeypoints + AddRegions            imagerepresentation.cpp:603-2047          (modsx_rep_add_views: one step)
//   LoadRegions / read_pre_extracted                     imagerepresentation.cpp:2139-2215, mods.cpp:236-241   (modsx_rep_append)
//   CorrespondenceBank::MatchImgReps(ImgRep1, ImgRep2)   correspondencebank.cpp:291-347            (reps_match_group)
// A slot owns the host region list, the [n][128] u8 descriptors in HBM and the PACKED TRAIN FORM of those descriptors and the
// regions' reprojected positions: what the train half of k_match_pack writes depends on the trains alone, so it is written once,
// when the slot changes, and every match that takes the slot as its train side starts from it (kernels_match.hip
// launch_match_pack_trains, MatchProblem::packed).  A representation is changed by one thread at a time; otherwise it is
// read-only and any context of its device may match against it, also at the same time.  The float classes (SURF, LIOP, DAISY,
// MROGH, learned vectors) and their grouped search are engine_reps_f32.hip, the binary classes (ORB, BRISK, FREAK) and theirs
// engine_reps_bin.hip; reps_match_group and reps_verify_task take all three kinds.
#include <math.h>
#include <algorithm>
#include "engine_api.hpp"

namespace mx {

bool rep_class_ok(int detector, int desc_type, int *det) {
  if (detector != MODSX_DET_HESSIAN && detector != MODSX_DET_MSER) return false;
  if (desc_type < 0 || desc_type > 3) return false;
  *det = detector == MODSX_DET_MSER ? 1 : 0;
  return true;
}

// the packed train form of a slot, rebuilt whole (the parity partition ranks a train among ALL trains of the slot) on c's stream
// and waited for: no match ever finds a slot whose pack is behind its descriptors
static int rep_repack(modsx_ctx *c, RepSlot &k) {
  const size_t n = k.regs.size();
  if (!n) return MODSX_OK;
  std::vector<double> pos(n * 2);
  for (size_t i = 0; i < n; i++) { pos[2 * i] = k.regs[i].reproj_kp.x; pos[2 * i + 1] = k.regs[i].reproj_kp.y; }
  if (!c->pos2.ensure(n * 16) || !k.pack.ensure(match_train_pack_bytes((int)n))) return MODSX_ERR_NOMEM;
  MX_HIP(hipMemcpyAsync(c->pos2.p, pos.data(), n * 16, hipMemcpyHostToDevice, c->stream));
  launch_match_pack_trains(c->stream, (const uint8_t *)k.desc.p, (int)n, (const double *)c->pos2.p, k.pack.p);
  MX_HIP(hipStreamSynchronize(c->stream));
  MX_HIP(hipGetLastError());
  return MODSX_OK;
}

int rep_add_views(modsx_ctx *c, modsx_rep *rep, const modsx_image *img, const modsx_ladder_step &st, const modsx_pair_params &pp) {
  CtxBusy busy(c);
  if (rep->dev != c->dev) { set_error("modsx_rep_add_views: the representation lives on another device"); return MODSX_ERR_ARG; }
  const int det = st.detector == MODSX_DET_MSER ? 1 : 0;
  DescSet ds;
  { const int rd = resolve_descs(pp, &st, ds); if (rd) return rd; }
  ClassSide ks[MODSX_MAX_DESC];
  for (int j = 0; j < ds.n; j++) { RepSlot &k = rep->slot[det][ds.type[j]]; ks[j] = {&k.regs, &k.cap, &k.desc}; }
  modsx_pair_params ps = pp;
  ps.detector = det ? MODSX_DET_MSER : MODSX_DET_HESSIAN;
  const size_t before = ks[0].regs->size();
  int rc = accumulate_views(c, ks, ds, img, st.views, st.nviews, ps);
  for (int j = 0; j < ds.n && !rc; j++) rc = rep_repack(c, rep->slot[det][ds.type[j]]);
  prof_collect(c);
  return rc ? rc : (int)(ks[0].regs->size() - before);
}

int rep_append(modsx_ctx *c, modsx_rep *rep, int det, int type, const modsx_region *regs, const uint8_t *descU8, int n) {
  CtxBusy busy(c);
  if (rep->dev != c->dev) { set_error("modsx_rep_append: the representation lives on another device"); return MODSX_ERR_ARG; }
  if (n == 0) return 0;
  RepSlot &k = rep->slot[det][type];
  const size_t base = k.regs.size();
  if (base + (size_t)n > 2000000) { set_error("modsx_rep_append: more than 2 000 000 regions in one class"); return MODSX_ERR_ARG; }
  while (k.cap < base + (size_t)n) k.cap *= 4;
  const ClassSide side = {&k.regs, &k.cap, &k.desc};
  { const int rg = class_side_reserve(c, side, base); if (rg) return rg; }
  MX_HIP(hipMemcpyAsync((uint8_t *)k.desc.p + base * 128, descU8, (size_t)n * 128, hipMemcpyHostToDevice, c->stream));
  MX_HIP(hipStreamSynchronize(c->stream));
  k.regs.insert(k.regs.end(), regs, regs + n);
  const int rc = rep_repack(c, k);
  return rc ? rc : n;
}

int rep_match_fginn(modsx_ctx *c, const modsx_rep *rep1, const modsx_rep *rep2, int det, int type, double ratio, double contradDist,
                    int nn, std::vector<modsx_tentative> &out) {
  if (rep1->dev != c->dev || rep2->dev != c->dev) { set_error("modsx_rep_match_fginn: a representation lives on another device"); return MODSX_ERR_ARG; }
  const RepSlot &q = rep1->slot[det][type], &t = rep2->slot[det][type];
  const uint8_t *d1 = (const uint8_t *)q.desc.p, *d2 = (const uint8_t *)t.desc.p;
  const int n1 = (int)q.regs.size(), n2 = (int)t.regs.size();
  const double *pos = nullptr;
  const void *pack = n2 ? t.pack.p : nullptr;
  return match_device_batch(c, 1, &d1, &n1, &d2, &n2, &pos, ratio, contradDist, nn, &out, nullptr, nullptr, nullptr, nullptr, &pack);
}

// MatchImgReps for the classes sel[0..nsel) of G <= MATCH_MAXB partners: one matcher launch set per class (problems with an
// empty side are left out by match_device_batch), rep1 the queries, the partners' packs the trains.  tents[g]->t[det][type]
// receives the class's tentatives of partner g; the other classes of tents[g] keep theirs.
int reps_match_group(modsx_ctx *c, const modsx_rep *rep1, const modsx_rep *const *reps2, int G, const modsx_rep_class_sel *sel, int nsel,
                     const modsx_pair_params &pp, RepTents *const *tents) {
  CtxBusy busy(c);
  if (G < 1 || G > MATCH_MAXB) { set_error("reps_match_group: group size"); return MODSX_ERR_ARG; }
  for (int s = 0; s < nsel; s++) {
    int det;
    const int type = sel[s].desc_type;
    if (rep_class_f32_ok(sel[s].detector, type, &det)) {
      // a float class: one grouped launch set of the f32 matcher (engine_reps_f32.hip)
      std::vector<modsx_tentative> out[MATCH_MAXB];
      const int rc = reps_f32_match_group(c, "modsx_match_reps", rep1, reps2, G, det, type, sel[s].ratio, pp.contradDist, pp.nn, out);
      if (rc) return rc;
      for (int g = 0; g < G; g++) tents[g]->f[det][type - MODSX_DESC_CAFFE] = std::move(out[g]);
      continue;
    }
    if (rep_class_bin_ok(sel[s].detector, type, &det)) {
      // a binary class: one grouped launch set of the Hamming search (engine_reps_bin.hip); `ratio` is its DistanceThreshold
      std::vector<modsx_tentative> out[MATCH_MAXB];
      const int rc = reps_bin_match_group(c, "modsx_match_reps", rep1, reps2, G, det, type, sel[s].ratio, out);
      if (rc) return rc;
      for (int g = 0; g < G; g++) tents[g]->b[det][type - MODSX_DESC_BRISK] = std::move(out[g]);
      continue;
    }
    if (!rep_class_ok(sel[s].detector, type, &det)) { set_error("modsx_match_reps: a class names a detector or descriptor type that does not exist"); return MODSX_ERR_ARG; }
    const RepSlot &q = rep1->slot[det][type];
    const uint8_t *d1[MATCH_MAXB], *d2[MATCH_MAXB];
    const double *pos[MATCH_MAXB];
    const void *pack[MATCH_MAXB];
    int n1[MATCH_MAXB], n2[MATCH_MAXB];
    std::vector<modsx_tentative> out[MATCH_MAXB];
    bool any = false;
    for (int g = 0; g < G; g++) {
      const RepSlot &t = reps2[g]->slot[det][type];
      d1[g] = (const uint8_t *)q.desc.p; n1[g] = (int)q.regs.size();
      d2[g] = (const uint8_t *)t.desc.p; n2[g] = (int)t.regs.size();
      pos[g] = nullptr;
      pack[g] = n2[g] ? t.pack.p : nullptr;
      any = any || (n1[g] > 0 && n2[g] > 0);
    }
    if (any) {
      const int rc = match_device_batch(c, G, d1, n1, d2, n2, pos, sel[s].ratio, pp.contradDist, pp.nn, out, nullptr, nullptr,
                                        fginn_db_for(c, type), nullptr, pack);
      if (rc) return rc;
    }
    for (int g = 0; g < G; g++) tents[g]->t[det][type] = std::move(out[g]);
  }
  prof_collect(c);
  return MODSX_OK;
}

// GetCorresponcesVector("All", "All") over the classes of `classes` (in map order: rep_class_rank) that are non-empty in either
// representation: the region lists as segments of the representations' own vectors (which must outlive the task), the tentatives
// re-based onto their concatenation.  res is reset to the zeroed result with H = -1.
void reps_verify_task(const modsx_rep *rep1, const modsx_rep *rep2, const RepClassList &classes, const RepTents &tents,
                      modsx_pair_result *res, int dev, VerifyTask &task) {
  memset(res, 0, sizeof *res);
  for (int i = 0; i < 9; i++) res->H[i] = -1;
  task.l1.clear(); task.l2.clear(); task.own.clear(); task.tents.clear();
  for (int i = 0; i < classes.n; i++) {
    const int d = classes.k[i].det, t = classes.k[i].type;
    const std::vector<modsx_region> &a = rep_slot_regions(rep1, d, t), &b = rep_slot_regions(rep2, d, t);
    if (a.empty() && b.empty()) continue;
    const int o1 = (int)task.l1.size(), o2 = (int)task.l2.size();
    task.l1.add(a); task.l2.add(b);
    const std::vector<modsx_tentative> &mine = t >= MODSX_DESC_BRISK ? tents.b[d][t - MODSX_DESC_BRISK] :
                                               t >= MODSX_DESC_CAFFE ? tents.f[d][t - MODSX_DESC_CAFFE] : tents.t[d][t];
    for (modsx_tentative tt : mine) {
      tt.q += o1; tt.t0 += o2;
      if (tt.t1 >= 0) tt.t1 += o2;
      if (tt.tj >= 0) tt.tj += o2;
      task.tents.push_back(tt);
    }
  }
  res->n_regions1 = (int)task.l1.size();
  res->n_regions2 = (int)task.l2.size();
  task.res = res; task.dev = dev;
}

}  // namespace mx

using namespace mx;

extern "C" {

modsx_rep *modsx_rep_create(modsx_ctx *ctx) {
  if (!ctx) { set_error("modsx_rep_create: null context"); return nullptr; }
  modsx_rep *rep = new modsx_rep();
  rep->dev = ctx->dev;
  return rep;
}

void modsx_rep_free(modsx_ctx *ctx, modsx_rep *rep) {
  if (!rep) return;
  hipSetDevice(ctx ? ctx->dev : rep->dev);
  for (int d = 0; d < 2; d++) for (int t = 0; t < 4; t++) { rep->slot[d][t].desc.release(); rep->slot[d][t].pack.release(); }
  rep_free_f32(rep);
  rep_free_bin(rep);
  delete rep;
}

int modsx_rep_add_views(modsx_ctx *ctx, modsx_rep *rep, const modsx_image *img, const modsx_ladder_step *step,
                        const modsx_pair_params *par) {
  if (!ctx || !rep || !img || !step || !par) { set_error("modsx_rep_add_views: null argument"); return MODSX_ERR_ARG; }
  if (!step->views || step->nviews <= 0) { set_error("modsx_rep_add_views: empty step"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  return rep_add_views(ctx, rep, img, *step, *par);
}

int modsx_rep_append(modsx_ctx *ctx, modsx_rep *rep, int detector, int desc_type, const modsx_region *regs, const void *desc, int dtype,
                     int n) {
  int det;
  if (!ctx || !rep || n < 0 || (n > 0 && (!regs || !desc)) || !rep_class_ok(detector, desc_type, &det)) {
    set_error("modsx_rep_append: bad argument (detector HessianAffine / MSER, descriptor type 0..3, n >= 0 regions with [n][128] descriptors)");
    return MODSX_ERR_ARG;
  }
  if (dtype != 0 && dtype != 1) { set_error("modsx_rep_append: dtype must be 0 (u8) or 1 (f32)"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  std::vector<uint8_t> conv;
  const uint8_t *u8 = (const uint8_t *)desc;
  if (dtype == 1 && n > 0) {
    conv.resize((size_t)n * 128);
    if (!desc_f32_to_u8((const float *)desc, conv.size(), conv.data())) {
      set_error("modsx_rep_append: descriptors must hold the integers 0..255 (SIFT-family quantisation)");
      return MODSX_ERR_ARG;
    }
    u8 = conv.data();
  }
  return rep_append(ctx, rep, det, desc_type, regs, u8, n);
}

int modsx_rep_class(modsx_ctx *ctx, const modsx_rep *rep, int detector, int desc_type, modsx_region **regs, unsigned char **desc_u8) {
  int det;
  if (!ctx || !rep || !rep_class_ok(detector, desc_type, &det)) { set_error("modsx_rep_class: bad argument"); return MODSX_ERR_ARG; }
  const RepSlot &k = rep->slot[det][desc_type];
  const size_t n = k.regs.size();
  if (regs) {
    *regs = (modsx_region *)malloc(sizeof(modsx_region) * std::max<size_t>(1, n));
    if (n) memcpy(*regs, k.regs.data(), sizeof(modsx_region) * n);
  }
  if (desc_u8) {
    *desc_u8 = (unsigned char *)malloc(std::max<size_t>(1, n * 128));
    if (n) {
      hipSetDevice(ctx->dev);
      if (hipMemcpyAsync(*desc_u8, k.desc.p, n * 128, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
          hipStreamSynchronize(ctx->stream) != hipSuccess) {
        free(*desc_u8); *desc_u8 = nullptr;
        if (regs) { free(*regs); *regs = nullptr; }
        set_error("modsx_rep_class: descriptor download failed");
        return MODSX_ERR_DEVICE;
      }
    }
  }
  return (int)n;
}

int modsx_rep_match_fginn(modsx_ctx *ctx, const modsx_rep *rep1, const modsx_rep *rep2, int detector, int desc_type, double ratio,
                          double contradDist, int nn, modsx_tentative **out) {
  int det;
  if (!ctx || !rep1 || !rep2 || !out || !rep_class_ok(detector, desc_type, &det)) { set_error("modsx_rep_match_fginn: bad argument"); return MODSX_ERR_ARG; }
  hipSetDevice(ctx->dev);
  std::vector<modsx_tentative> t;
  const int rc = rep_match_fginn(ctx, rep1, rep2, det, desc_type, ratio, contradDist, nn, t);
  if (rc) return rc;
  *out = (modsx_tentative *)malloc(sizeof(modsx_tentative) * std::max<size_t>(1, t.size()));
  if (!t.empty()) memcpy(*out, t.data(), sizeof(modsx_tentative) * t.size());
  return (int)t.size();
}

}  // extern "C"
