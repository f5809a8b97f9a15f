/* oracle_mser.cpp -- TEST INFRASTRUCTURE ONLY: CPU restatement of the reference's MSER detector (SURVEY.md rows
 * E1, E2).  PINNED: the reference's MSER sources compile in place behind two stand-in OpenCV headers (oracle/Makefile,
 * _ref/libmser_ref.so) and tests/test_mser_ref_cpu.py holds this file to them bit for bit, for images of 64 pixels and more (the
 * reference faults on tiny ones; below that this file is the only check).  It follows the reference's own data structures step by
 * step (tagged label words, packed minimal regions, per-level pixel/border histograms) so that the product's
 * independent implementation (mods_amd/csrc/mser.cpp, plain union-find) can be cross-checked against it.
 *
 * Reference (detectors/mser/extrema/):
 *   DetectMSERs 6-arg             extrema.cpp:284-473 (doOnNormal branch :393-468), prepareKeysForExport :31-90
 *   getRLEExtrema                 libExtrema.cpp:539-560; extremaPrepareImage :341-353; extremaInvertImage :368-372
 *   CalcHistogram / BinSortPixels / InvertImageAndHistogram    sortPixels.cpp:76-155
 *   GetExtrema                    getExtrema.cpp:390-437 (GetLabelled :217-265, FindEquivLabel :185-215,
 *                                 ConsRegion :172-176, InsMarkPixel :145-171, UpgradeRegion :103-142, MergeRegions :267-361)
 *   FastSetOptThresholds4StableRegion + SuppresOverlappingTresholds4StableRegions   optThresh.cpp:15-166
 *   RegionBoundaries              boundary.cpp:107-209 (the extended boundary of the 4-connected component of
 *                                 {pixel <= thresh} that holds the region's first pixel); ReducedBoundary2RLE
 *                                 libExtrema.cpp:161-185; RLE2Ellipse :117-159
 *   Matrix2::schur_sym / sqrt     utls/matrix.cpp:185-217, 115-119
 */
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "oracle.h"

namespace {

typedef uint64_t Label;
const Label LABEL_MASK = ~(Label)3, LABELPTR_MASK = 3, MINREG_FLAG = 1, REGION_FLAG = 2;
const Label REGION_SIZE_MASK = 0x1fffc;
const int REGION_SIZE_SHIFT = 2, BORDER_SIZE_SHIFT = 17;

struct Thresh { int thresh, pos, margin; };
struct Region {
  int minimum_int, maximum_int, pixel_total, border_total;
  unsigned minimum_pos;            /* offset of the label word that became the region (padded coordinates) */
  int pixels[256], borders[256];
  std::vector<Thresh> thr;
  bool linked;                     /* still in the `regions` list */
};
struct ThreshPar { int min_size, min_size_int, max_size; double min_margin; bool relative_margin; int invert; };

struct Extrema {
  int rows, cols, g_cols;          /* real size; g_cols = cols + 2 */
  std::vector<unsigned char> img;  /* padded (rows+2) x (cols+2) */
  std::vector<unsigned> data[256]; /* pixel offsets per intensity, raster order (BinSortPixels) */
  std::vector<Label> labels;
  std::vector<Region *> regions;   /* creation order = LinkInsLastLL order */
  ThreshPar tp;
  /* a label word holds: 0 | pointer to another label word ((slot + 1) << 2) | packed minimal region (bit 0) |
   * region reference ((index << 2) | 2); the reference stores raw pointers in the same three forms */
  std::vector<Region *> pool;
  int labelled[4], label_num, border_num;

  ~Extrema() { for (Region *r : pool) delete r; }
  static Label ptr(int slot) { return ((Label)slot + 1) << 2; }
  static int slot_of(Label v) { return (int)(v >> 2) - 1; }
  Region *region_of(Label v) { return pool[(size_t)(v >> 2)]; }

  int find_equiv(int label) {      /* FindEquivLabel: `label` is a slot whose word is a pointer */
    int p = slot_of(labels[label]);
    if (labels[p] & LABELPTR_MASK) return p;
    do p = slot_of(labels[p]); while ((labels[p] & LABELPTR_MASK) == 0);
    const int fin = p;
    p = label;
    while ((labels[p] & LABELPTR_MASK) == 0) {
      const int nx = slot_of(labels[p]);
      labels[label] = ptr(fin);
      label = nx;
      p = nx;
    }
    return fin;
  }
  void get_labelled(unsigned ofs) {   /* getExtrema.cpp:217-265: up, left, right, down; resolved roots compared pairwise */
    const int nb[4] = {(int)ofs - g_cols, (int)ofs - 1, (int)ofs + 1, (int)ofs + g_cols};
    int res[4] = {-1, -1, -1, -1};
    label_num = 0; border_num = 0;
    for (int k = 0; k < 4; k++) {
      if (labels[nb[k]] == 0) continue;
      int l = nb[k];
      if ((labels[l] & LABELPTR_MASK) == 0) l = find_equiv(l);
      res[k] = l;
      bool dup = false;
      for (int q = 0; q < k; q++) dup = dup || res[q] == l;
      if (!dup) labelled[label_num++] = l;
      border_num++;
    }
    border_num = 2 * border_num;
  }

  Region *upgrade(int slot, int intensity) {
    Region *r = new Region();
    memset(r->pixels, 0, sizeof r->pixels);
    memset(r->borders, 0, sizeof r->borders);
    const Label min_reg = labels[slot] & LABEL_MASK;
    r->pixel_total = (int)((min_reg & REGION_SIZE_MASK) >> REGION_SIZE_SHIFT);
    r->border_total = (int)(min_reg >> BORDER_SIZE_SHIFT);
    r->minimum_pos = (unsigned)slot;
    r->minimum_int = r->maximum_int = intensity;
    r->pixels[intensity] = r->pixel_total;
    r->borders[intensity] = r->border_total;
    r->linked = true;
    pool.push_back(r);
    regions.push_back(r);
    labels[slot] = ((Label)(pool.size() - 1) << 2) | REGION_FLAG;
    return r;
  }
  void ins_mark_pixel(int slot, unsigned ofs, int intensity) {
    labels[ofs] = ptr(slot);
    if (labels[slot] & MINREG_FLAG) {
      labels[slot] += 0x00080004 - ((Label)border_num << BORDER_SIZE_SHIFT);
      if ((int)(labels[slot] & REGION_SIZE_MASK) >= tp.min_size_int) upgrade(slot, intensity);
    } else {
      Region *r = region_of(labels[slot]);
      r->maximum_int = intensity;
      r->pixel_total++;
      r->border_total += 4 - border_num;
      r->pixels[intensity]++;
      r->borders[intensity] += 4 - border_num;
    }
  }
  void unlink(Region *r) { r->linked = false; }

  void suppress_overlapping(Region *r, const int *cum) {   /* optThresh.cpp:15-65 */
    std::vector<Thresh> &t = r->thr;
    if (t.empty()) return;
    for (int i = 0; i < (int)t.size(); i++) {
      while (i >= 0 && i + 1 < (int)t.size()) {
        const int nx = i + 1;
        if ((t[i].pos + t[i].margin < t[nx].thresh) && (t[i].thresh < t[nx].pos)) break;
        if (t[nx].margin <= t[i].margin) t.erase(t.begin() + nx);
        else { t.erase(t.begin() + i); i--; break; }
      }
    }
    for (int i = 0; i < (int)t.size(); i++) {
      while (i + 1 < (int)t.size()) {
        const int nx = i + 1;
        if (t[i].pos + t[i].margin < t[nx].pos) break;
        if (cum[t[nx].thresh] - cum[t[i].thresh] <= 0.1 * cum[t[i].thresh]) {
          t[i].margin = t[nx].pos - t[i].pos + t[nx].margin;
          t[i].thresh = t[i].pos + t[i].margin / 2;
          t.erase(t.begin() + nx);
        } else break;
      }
    }
  }
  void set_opt_thresholds(Region *r) {                     /* optThresh.cpp:69-166 */
    if (r->pixel_total < tp.min_size) return;
    const int invertCons = tp.invert ? 255 : 0, invertMulti = tp.invert ? -1 : 1;
    int *cumA = r->pixels, *cumB = r->borders;
    for (int i = r->minimum_int + 1; i <= r->maximum_int; i++) { r->pixels[i] += r->pixels[i - 1]; r->borders[i] += r->borders[i - 1]; }
    int up, localMaxMargin = -1, localMaxPos = -1;
    int i = r->minimum_int;
    auto emit = [&]() {
      Thresh t;
      t.thresh = localMaxPos + localMaxMargin / 2;
      if (cumA[t.thresh] <= tp.max_size && cumA[t.thresh] > tp.min_size) {
        t.pos = localMaxPos; t.margin = localMaxMargin;
        r->thr.push_back(t);
      }
    };
    do {
      const int area_i = cumA[i], radius_i = cumB[i];
      up = int(i + tp.min_margin);
      if (up > r->maximum_int) break;
      while ((cumA[up] - area_i < radius_i) && (up < r->maximum_int)) up++;
      const int margin = up - i;
      double quality = (double)margin;
      if (tp.relative_margin) quality /= invertCons + invertMulti * (i + (margin / 2));
      if (quality > tp.min_margin && margin >= localMaxMargin) { localMaxMargin = margin; localMaxPos = i; }
      else {
        if (localMaxPos >= 0) { emit(); localMaxPos = -1; }
        localMaxMargin = margin;
      }
      i++;
    } while (up < r->maximum_int);
    if (localMaxPos >= 0) emit();
    suppress_overlapping(r, cumA);
  }

  void merge_regions(unsigned ofs, int intensity) {        /* getExtrema.cpp:267-361 */
    unsigned maxSize = 0;
    int maxLabel = labelled[0], num_large = 0;
    for (int i = 0; i < label_num; i++) {
      const Label w = labels[labelled[i]];
      if (!(w & MINREG_FLAG)) {
        Region *region = region_of(w);
        const unsigned size = (unsigned)(region->pixel_total - region->pixels[intensity]);
        num_large++;
        if (size > maxSize) { maxSize = size; maxLabel = labelled[i]; }
      }
    }
    if (!num_large) {
      for (int i = 1; i < label_num; i++) {
        labels[maxLabel] += (labels[labelled[i]] & LABEL_MASK);
        labels[labelled[i]] = ptr(maxLabel);
      }
    } else {
      const bool max_has_minstats = (labels[maxLabel] & MINREG_FLAG) != 0;
      Region *maxRegion = max_has_minstats ? nullptr : region_of(labels[maxLabel]);
      for (int i = 0; i < label_num; i++) {
        const int label = labelled[i];
        if (label == maxLabel) continue;
        const Label min_reg = labels[label];
        const bool merging_min_reg = (min_reg & MINREG_FLAG) != 0;
        Region *region = merging_min_reg ? nullptr : region_of(min_reg);
        labels[label] = ptr(maxLabel);
        int pixel_total, border_total;
        if (merging_min_reg) {
          pixel_total = (int)((min_reg & REGION_SIZE_MASK) >> REGION_SIZE_SHIFT);
          border_total = (int)(min_reg >> BORDER_SIZE_SHIFT);
        } else { pixel_total = region->pixel_total; border_total = region->border_total; }
        if (max_has_minstats) labels[maxLabel] += ((Label)pixel_total << REGION_SIZE_SHIFT) + ((Label)border_total << BORDER_SIZE_SHIFT);
        else {
          maxRegion->pixel_total += pixel_total;
          maxRegion->border_total += border_total;
          maxRegion->pixels[intensity] += pixel_total;
          maxRegion->borders[intensity] += border_total;
        }
        if (!merging_min_reg) {
          if (!tp.relative_margin && (intensity - region->minimum_int + 1) <= tp.min_margin) unlink(region);
          else {
            region->maximum_int = intensity;
            set_opt_thresholds(region);
            if (region->thr.empty()) unlink(region);
          }
        }
      }
    }
    ins_mark_pixel(maxLabel, ofs, intensity);
  }

  void run(bool invert, int min_size, double max_area, double min_margin, bool relative) {
    tp.min_size = min_size;
    tp.min_size_int = std::min(10000, min_size) * 4;
    tp.max_size = (int)((double)(cols) * (rows) * max_area);   /* (img->cols()-2)*(img->rows()-2) of the padded array */
    tp.min_margin = relative ? min_margin / 100.0 : min_margin;
    tp.invert = invert; tp.relative_margin = relative;
    labels.assign((size_t)(rows + 2) * g_cols, 0);
    for (int i = 0; i < 256; i++)
      for (unsigned ofs : data[i]) {
        get_labelled(ofs);
        if (label_num == 0) labels[ofs] = 0x00080004 | MINREG_FLAG;                 /* ConsRegion */
        else if (label_num == 1) ins_mark_pixel(labelled[0], ofs, i);
        else merge_regions(ofs, i);
      }
    int root = g_cols + 1;
    if ((labels[root] & LABELPTR_MASK) == 0) root = find_equiv(root);
    if (labels[root] & REGION_FLAG) set_opt_thresholds(region_of(labels[root]));
  }
};

}  // namespace

namespace {

struct Run { int line, col1, col2; };

/* the 4-connected component of {img <= thresh} that holds `seed` (RegionBoundaries + ReducedBoundary2RLE yield its
 * row runs in raster order) */
static void component_runs(const Extrema &E, unsigned seed, int thresh, std::vector<unsigned char> &mark,
                           std::vector<unsigned> &stack, std::vector<unsigned> &pix, std::vector<Run> &rle) {
  pix.clear(); stack.clear(); rle.clear();
  const int gc = E.g_cols;
  auto inside = [&](unsigned o) {
    const int r = (int)(o / gc), c = (int)(o % gc);
    return r >= 1 && r <= E.rows && c >= 1 && c <= E.cols && E.img[o] <= thresh && !mark[o];
  };
  if (!inside(seed)) return;
  mark[seed] = 1; stack.push_back(seed);
  while (!stack.empty()) {
    const unsigned o = stack.back(); stack.pop_back();
    pix.push_back(o);
    const unsigned nb[4] = {o + gc, o - gc, o + 1, o - 1};
    for (unsigned q : nb) if (inside(q)) { mark[q] = 1; stack.push_back(q); }
  }
  std::sort(pix.begin(), pix.end());
  for (size_t i = 0; i < pix.size();) {
    size_t j = i;
    while (j + 1 < pix.size() && pix[j + 1] == pix[j] + 1) j++;
    Run r;
    r.line = (int)(pix[i] / gc) - 1; r.col1 = (int)(pix[i] % gc) - 1; r.col2 = (int)(pix[j] % gc) - 1;
    rle.push_back(r);
    i = j + 1;
  }
  for (unsigned o : pix) mark[o] = 0;
}

static void rle2ellipse(const std::vector<Run> &rle, double &barX, double &barY, double &sumX2, double &sumXY, double &sumY2) {
  double area = 0, sumX = 0, sumY = 0;
  for (const Run &q : rle) {
    const double line = q.line, m = q.col1, n = 1 + q.col2;
    sumX += (n * n - m * m) / 2;
    sumY += (n - m) * (2 * line + 1) / 2;
    area += n - m;
  }
  barX = (double)sumX / (double)area;
  barY = (double)sumY / (double)area;
  sumX2 = sumY2 = sumXY = 0;
  for (const Run &q : rle) {
    const double line = q.line - barY, m = q.col1 - barX, n = 1 + q.col2 - barX;
    const double l2 = line * line, m2 = m * m, n2 = n * n;
    sumX2 += (n2 * n - m2 * m) / 3;
    sumY2 += (n - m) * (3 * l2 + 3 * line + 1) / 3;
    sumXY += -.25 * (m2 - n2) * (2 * line + 1);
  }
  sumX2 /= (double)area; sumY2 /= (double)area; sumXY /= (double)area;
}

/* A = U * sqrt(T) * U^T with C = U T U^T from Matrix2::schur_sym (matrix.cpp:185-217) */
static void sqrt_sym2(double c00, double c01, double c11, double *A) {
  double t, r;
  if (c01 != 0) {
    r = double(c11 - c00) / (2 * c01);
    if (r >= 0) t = 1.0 / (r + ::sqrt(1 + r * r));
    else t = -1.0 / (-r + ::sqrt(1 + r * r));
    r = 1.0 / ::sqrt(1 + t * t);
    t = t * r;
  } else { r = 1; t = 0; }
  const double Q[2][2] = {{r, t}, {-t, r}};
  const double Cm[2][2] = {{c00, c01}, {c01, c11}};
  /* T = Q^T * C * Q (operator* = plain row-by-column products), off-diagonal zeroed */
  double QtC[2][2], T[2][2];
  for (int i = 0; i < 2; i++) for (int j = 0; j < 2; j++) QtC[i][j] = Q[0][i] * Cm[0][j] + Q[1][i] * Cm[1][j];
  for (int i = 0; i < 2; i++) for (int j = 0; j < 2; j++) T[i][j] = QtC[i][0] * Q[0][j] + QtC[i][1] * Q[1][j];
  T[0][1] = 0; T[1][0] = 0;
  const double S[2][2] = {{::sqrt(T[0][0]), ::sqrt(T[0][1])}, {::sqrt(T[1][0]), ::sqrt(T[1][1])}};
  double QS[2][2];
  for (int i = 0; i < 2; i++) for (int j = 0; j < 2; j++) QS[i][j] = Q[i][0] * S[0][j] + Q[i][1] * S[1][j];
  for (int i = 0; i < 2; i++) for (int j = 0; j < 2; j++) A[i * 2 + j] = QS[i][0] * Q[j][0] + QS[i][1] * Q[j][1];
}

}  // namespace

extern "C" {

/* DetectMSERs (doOnNormal), extrema.cpp:284-300, 393-468.  mode: orc detection_mode values as for the Hessian
 * detector.  Returns the number of keypoints (<= cap). */
int orc_detect_msers(const float *img, int rows, int cols, int min_size, double max_area, double min_margin_par,
                     int relative, int mode, int reg_number, double rel_threshold_par, double rel_reg_number_par, double tilt,
                     double zoom, orc_keypoint *out, int cap) {
  /* ExtremaParams::rel_threshold and rel_reg_number are floats (extremaParams.h:68-70): 0.7 is 0.699999988 there, which moves
   * floor(0.7 * 10) from 7 to 6 and the RELATIVE_TH probe below a tie at 70 % of the top margin */
  const float rel_threshold = (float)rel_threshold_par, rel_reg_number = (float)rel_reg_number_par;
  if ((tilt > 2.0) || (zoom < 0.5)) reg_number = (int)floor(zoom * 2.0 * reg_number / tilt);
  const double min_margin = (mode != 0) ? 1.0 : min_margin_par;   /* FIXED_TH = 0 */
  Extrema E;
  E.rows = rows; E.cols = cols; E.g_cols = cols + 2;
  E.img.assign((size_t)(rows + 2) * E.g_cols, 0);
  for (int r = 0; r < rows; r++)
    for (int c = 0; c < cols; c++) E.img[(size_t)(r + 1) * E.g_cols + c + 1] = (unsigned char)img[(size_t)r * cols + c];
  std::vector<orc_keypoint> keys;
  std::vector<unsigned char> mark((size_t)(rows + 2) * E.g_cols, 0);
  std::vector<unsigned> stack, pix;
  std::vector<Run> rle;
  for (int pol = 0; pol < 2; pol++) {
    if (pol == 1)
      for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) { unsigned char &v = E.img[(size_t)(r + 1) * E.g_cols + c + 1]; v = 255 - v; }
    for (int i = 0; i < 256; i++) E.data[i].clear();
    for (int r = 0; r < rows; r++)
      for (int c = 0; c < cols; c++) {
        const unsigned ofs = (unsigned)((r + 1) * E.g_cols + c + 1);
        E.data[E.img[ofs]].push_back(ofs);
      }
    for (Region *r : E.pool) delete r;
    E.pool.clear(); E.regions.clear();
    E.run(pol == 1, min_size, max_area, min_margin, relative != 0);
    for (Region *r : E.regions) {
      if (!r->linked) continue;
      for (const Thresh &t : r->thr) {
        if (t.thresh >= 255) continue;   /* RegionBoundaries skips level 255; the reference would dereference NULL */
        component_runs(E, r->minimum_pos, t.thresh, mark, stack, pix, rle);
        if (rle.empty()) continue;
        double bx, by, sx2, sxy, sy2, A[4];
        rle2ellipse(rle, bx, by, sx2, sxy, sy2);
        sqrt_sym2(sx2, sxy, sy2, A);
        orc_keypoint k;
        memset(&k, 0, sizeof k);
        k.x = bx; k.y = by; k.a11 = A[0]; k.a12 = A[1]; k.a21 = A[2]; k.a22 = A[3];
        k.s = 1.0; k.response = t.margin; k.sub_type = pol == 0 ? 21 : 20;
        keys.push_back(k);
      }
    }
  }
  /* prepareKeysForExport, extrema.cpp:31-90 */
  if (!keys.empty() && mode != 0) {
    auto cmp = [](const orc_keypoint &a, const orc_keypoint &b) { return fabs(a.response) > fabs(b.response); };
    std::sort(keys.begin(), keys.end(), cmp);
    const double maxResponse = fabs(keys[0].response);
    const int regNumber = (int)keys.size();
    orc_keypoint tmp = keys[0];
    switch (mode) {
      case 1: {  /* RELATIVE_TH */
        tmp.response = maxResponse * rel_threshold;
        keys.resize(std::lower_bound(keys.begin(), keys.end(), tmp, cmp) - keys.begin());
        break; }
      case 2: if ((reg_number < regNumber) && (reg_number >= 0)) keys.resize(reg_number); break;   /* FIXED_REG_NUMBER */
      case 3: keys.resize((int)floor(rel_reg_number * (double)keys.size())); break;                  /* RELATIVE_REG_NUMBER */
      case 4: {  /* NOT_LESS_THAN_REGIONS */
        tmp.response = min_margin;
        const int fixTh = (int)(std::lower_bound(keys.begin(), keys.end(), tmp, cmp) - keys.begin());
        if (fixTh < reg_number) keys.resize(std::min(reg_number, regNumber));
        else keys.resize(std::min(fixTh, regNumber));
        break; }
      default: break;
    }
  }
  const int n = (int)std::min<size_t>(keys.size(), (size_t)cap);
  for (int i = 0; i < n; i++) out[i] = keys[i];
  return (int)keys.size();
}
}
