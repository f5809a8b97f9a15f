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
// engine_reps_bin.hip; reps_match_group and reps_verify_task take all three kinds.  What the kinds share is here in one copy: the
// class table (which (detector, descriptor) pairs are classes, of which kind, in which slot and in which order) and the store of
// the float and the binary slots (slot_release, slot_reserve, slot_zero_again, slot_download).
#include <math.h>
#include <algorithm>
#include "engine_api.hpp"

namespace mx {

// ---- the class table: what GetCorresponcesVector("All", "All") (correspondencebank.cpp:117-179) iterates over ----
// the twelve descriptor names in std::map order: BRISK, CAFFE, DAISY, FREAK, HalfRootSIFT, HalfSIFT, LIOP, MROGH, ORB, RootSIFT,
// SIFT, SURF; the four detector names: HessianAffine, MSER, ORB, SURF
static const int DESC_ORDER[12] = {MODSX_DESC_BRISK, MODSX_DESC_CAFFE, MODSX_DESC_DAISY, MODSX_DESC_FREAK, MODSX_DESC_HALF_ROOT_SIFT,
                                   MODSX_DESC_HALF_SIFT, MODSX_DESC_LIOP, MODSX_DESC_MROGH, MODSX_DESC_ORB, MODSX_DESC_ROOT_SIFT,
                                   MODSX_DESC_SIFT, MODSX_DESC_SURF};
static const int DET_ORDER[4] = {MODSX_DET_HESSIAN, MODSX_DET_MSER, MODSX_DET_ORB, MODSX_DET_SURF};
// per kind (REP_U8, REP_F32, REP_BIN) and detector place: the slot index inside the kind, -1: the kind has no class of that detector
static const int SLOT_OF[3][4] = {{0, 1, -1, -1}, {0, 1, -1, 2}, {0, 1, 2, 3}};
static int kind_of(int type) {
  if (type >= MODSX_DESC_SIFT && type <= MODSX_DESC_HALF_ROOT_SIFT) return REP_U8;
  if (type >= MODSX_DESC_CAFFE && type <= MODSX_DESC_SURF) return REP_F32;
  return type >= MODSX_DESC_BRISK && type <= MODSX_DESC_ORB ? REP_BIN : -1;
}
static int place_in(const int *order, int n, int v) {
  for (int i = 0; i < n; i++) if (order[i] == v) return i;
  return -1;
}

bool rep_class_id(int detector, int desc_type, RepClassId *id) {
  const int kind = kind_of(desc_type), dp = place_in(DET_ORDER, 4, detector);
  if (kind < 0 || dp < 0 || SLOT_OF[kind][dp] < 0) return false;
  *id = {kind, SLOT_OF[kind][dp], desc_type, place_in(DESC_ORDER, 12, desc_type) * 4 + dp};
  return true;
}
int rep_class_detector(const RepClassId &k) { return DET_ORDER[k.order % 4]; }
void rep_classes(RepClassList &l, unsigned kinds) {
  RepClassId k;
  for (int o = 0; o < REP_ORDERS; o++)
    if (rep_class_id(DET_ORDER[o % 4], DESC_ORDER[o / 4], &k) && (kinds >> k.kind & 1)) l.add(k);
}
int rep_class_order(int detector, int desc_type) {
  RepClassId k;
  return rep_class_id(detector, desc_type, &k) ? k.order : -1;
}
// the same order over the names that are not binary, with the float slots' three detectors for every one of them
int rep_class_rank(int detector, int desc_type) {
  const int kind = kind_of(desc_type), dp = place_in(DET_ORDER, 4, detector);
  if (kind < 0 || kind == REP_BIN || dp < 0 || SLOT_OF[REP_F32][dp] < 0) return -1;
  int names = 0;
  for (int i = 0; DESC_ORDER[i] != desc_type; i++) names += kind_of(DESC_ORDER[i]) != REP_BIN;
  return names * 3 + SLOT_OF[REP_F32][dp];
}
const std::vector<modsx_region> &rep_class_regions(const modsx_rep *rep, const RepClassId &k) {
  if (k.kind == REP_BIN) return rep->bslot[k.det][k.type - MODSX_DESC_BRISK].regs;
  if (k.kind == REP_F32) return rep->fslot[k.det][k.type - MODSX_DESC_CAFFE].regs;
  return rep->slot[k.det][k.type].regs;
}

// ---- the store of the float and the binary slots (RepRows) ----
void slot_release(RepRows &k) {
  k.rows.release(); k.pos.release();
  k.cap = 0; k.capW = 0;
}

int slot_reserve(modsx_ctx *c, RepRows &k, size_t rows, int W, bool isFloat) {
  if (k.cap && k.capW != W) {
    if (!k.regs.empty()) { set_error(std::string(isFloat ? "a float" : "a binary") + " class holds rows of another kernel width"); return MODSX_ERR_ARG; }
    slot_release(k);
  }
  if (rows <= k.cap) return MODSX_OK;
  size_t cap = k.cap ? k.cap : isFloat ? MODSX_REP_F32_FIRST_ROWS : MODSX_REP_BIN_FIRST_ROWS;
  while (cap < rows) cap *= 4;
  DevBuf nr, np;
  if (!nr.ensure(cap * W * 4) || (isFloat && !np.ensure(cap * 16))) { nr.release(); np.release(); return MODSX_ERR_NOMEM; }
  const size_t n = k.regs.size();
  hipError_t e = hipMemsetAsync(nr.p, 0, cap * W * 4, c->stream);
  if (e == hipSuccess && n) e = hipMemcpyAsync(nr.p, k.rows.p, n * W * 4, hipMemcpyDeviceToDevice, c->stream);
  if (e == hipSuccess && n && isFloat) e = hipMemcpyAsync(np.p, k.pos.p, n * 16, hipMemcpyDeviceToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) { nr.release(); np.release(); }
  MX_HIP(e);
  k.rows.release(); k.pos.release();
  k.rows = nr; k.pos = np; k.cap = cap; k.capW = W;
  return MODSX_OK;
}

hipError_t slot_zero_again(modsx_ctx *c, RepRows &k, size_t base, int n) {
  hipError_t e = hipMemsetAsync((uint32_t *)k.rows.p + base * k.capW, 0, (size_t)n * k.capW * 4, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  return e;
}

int slot_download(modsx_ctx *c, const char *fn, const RepRows &k, size_t widthBytes, modsx_region **regs, void **rows) {
  CtxBusy busy(c);
  const std::string f(fn);
  const size_t n = k.regs.size();
  if (regs) *regs = nullptr;
  if (rows) {
    *rows = malloc(std::max<size_t>(4, n * widthBytes));
    if (!*rows) { set_error(f + ": out of memory"); return MODSX_ERR_NOMEM; }
    if (n) {      // a row is its values in order, zero behind widthBytes
      hipError_t e = hipMemcpy2DAsync(*rows, widthBytes, k.rows.p, (size_t)k.W * 4, widthBytes, n, hipMemcpyDeviceToHost, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
      if (e != hipSuccess) { free(*rows); *rows = nullptr; set_error(f + ": row download failed"); return MODSX_ERR_DEVICE; }
    }
  }
  if (regs) {
    *regs = to_malloc(k.regs);
    if (!*regs) {
      if (rows) { free(*rows); *rows = nullptr; }
      set_error(f + ": out of memory");
      return MODSX_ERR_NOMEM;
    }
  }
  return (int)n;
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

// one u8 class of G partners: one matcher launch set (problems with an empty side are left out by match_device_batch), rep1 the
// queries, the partners' packs the trains
static int reps_u8_match_group(modsx_ctx *c, const modsx_rep *rep1, const modsx_rep *const *reps2, int G, int det, int type, double ratio,
                               const modsx_pair_params &pp, std::vector<modsx_tentative> *out) {
  const RepSlot &q = rep1->slot[det][type];
  const uint8_t *d1[MATCH_MAXB], *d2[MATCH_MAXB];
  const double *pos[MATCH_MAXB];
  const void *pack[MATCH_MAXB];
  int n1[MATCH_MAXB], n2[MATCH_MAXB];
  bool any = false;
  for (int g = 0; g < G; g++) {
    const RepSlot &t = reps2[g]->slot[det][type];
    d1[g] = (const uint8_t *)q.desc.p; n1[g] = (int)q.regs.size();
    d2[g] = (const uint8_t *)t.desc.p; n2[g] = (int)t.regs.size();
    pos[g] = nullptr;
    pack[g] = n2[g] ? t.pack.p : nullptr;
    any = any || (n1[g] > 0 && n2[g] > 0);
  }
  if (!any) return MODSX_OK;
  return match_device_batch(c, G, d1, n1, d2, n2, pos, ratio, pp.contradDist, pp.nn, out, nullptr, nullptr, fginn_db_for(c, type), nullptr, pack);
}

// MatchImgReps for the classes sel[0..nsel) of G <= MATCH_MAXB partners: one launch set per class -- the u8 matcher, the grouped
// f32 matcher (engine_reps_f32.hip) or the grouped Hamming search (engine_reps_bin.hip; `ratio` is its DistanceThreshold).
// tents[g]->of[the class's order] receives the class's tentatives of partner g; the other classes of tents[g] keep theirs.
int reps_match_group(modsx_ctx *c, const modsx_rep *rep1, const modsx_rep *const *reps2, int G, const modsx_rep_class_sel *sel, int nsel,
                     const modsx_pair_params &pp, RepTents *const *tents) {
  CtxBusy busy(c);
  if (G < 1 || G > MATCH_MAXB) { set_error("reps_match_group: group size"); return MODSX_ERR_ARG; }
  for (int s = 0; s < nsel; s++) {
    RepClassId k;
    if (!rep_class_id(sel[s].detector, sel[s].desc_type, &k)) { set_error("modsx_match_reps: a class names a detector or descriptor type that does not exist"); return MODSX_ERR_ARG; }
    std::vector<modsx_tentative> out[MATCH_MAXB];
    const int rc = k.kind == REP_F32 ? reps_f32_match_group(c, "modsx_match_reps", rep1, reps2, G, k.det, k.type, sel[s].ratio, pp.contradDist, pp.nn, out)
                 : k.kind == REP_BIN ? reps_bin_match_group(c, "modsx_match_reps", rep1, reps2, G, k.det, k.type, sel[s].ratio, out)
                                     : reps_u8_match_group(c, rep1, reps2, G, k.det, k.type, sel[s].ratio, pp, out);
    if (rc) return rc;
    for (int g = 0; g < G; g++) tents[g]->of[k.order] = std::move(out[g]);
  }
  prof_collect(c);
  return MODSX_OK;
}

// GetCorresponcesVector("All", "All") over the classes of `classes` (in map order: RepClassId::order) that are non-empty in either
// representation: the region lists as segments of the representations' own vectors (which must outlive the task), the tentatives
// re-based onto their concatenation.  res is reset to the zeroed result with H = -1.
void reps_verify_task(const modsx_rep *rep1, const modsx_rep *rep2, const RepClassList &classes, const RepTents &tents,
                      modsx_pair_result *res, int dev, VerifyTask &task) {
  memset(res, 0, sizeof *res);
  for (int i = 0; i < 9; i++) res->H[i] = -1;
  task.l1.clear(); task.l2.clear(); task.own.clear(); task.tents.clear();
  for (int i = 0; i < classes.n; i++) {
    const RepClassId &k = classes.k[i];
    const std::vector<modsx_region> &a = rep_class_regions(rep1, k), &b = rep_class_regions(rep2, k);
    if (a.empty() && b.empty()) continue;
    const int o1 = (int)task.l1.size(), o2 = (int)task.l2.size();
    task.l1.add(a); task.l2.add(b);
    for (modsx_tentative tt : tents.of[k.order]) {
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

int modsx_rep_class_rank(int detector, int desc_type) { return rep_class_rank(detector, desc_type); }
int modsx_rep_class_order(int detector, int desc_type) { return rep_class_order(detector, desc_type); }

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
  for (auto &byDet : rep->fslot) for (RepSlotF &k : byDet) slot_release(k);
  for (auto &byDet : rep->bslot) for (RepSlotB &k : byDet) slot_release(k);
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
  if (regs) *regs = to_malloc(k.regs);
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
  *out = to_malloc(t);
  return (int)t.size();
}

}  // extern "C"
