// views_plan.cpp -- the host arithmetic of view synthesis (views_plan.hpp): no device, no context.
#include <math.h>
#include <string.h>
#include <algorithm>
#include "views_plan.hpp"

namespace mx {

// cv::warpAffine inverts the forward 2x3 matrix in f64 before the pixel loop (imgwarp.cpp)
static void invert_affine(const double *Min, double *M) {
  for (int i = 0; i < 6; i++) M[i] = Min[i];
  double D = M[0] * M[4] - M[1] * M[3];
  D = D != 0 ? 1. / D : 0;
  double A11 = M[4] * D, A22 = M[0] * D;
  M[0] = A11; M[1] *= -D;
  M[3] *= -D; M[4] = A22;
  double b1 = -M[0] * M[2] - M[1] * M[5];
  double b2 = -M[3] * M[2] - M[4] * M[5];
  M[2] = b1; M[5] = b2;
}

int plan_view(int rows, int cols, const modsx_view &v, ViewPlan &P) {
  double tilt = v.tilt;
  const double phi = v.phi, zoom = v.zoom, InitSigma = v.InitSigma;
  int zoomed = 0;
  bool vertical_tilt = false;
  if (tilt < 0) { tilt = -tilt; vertical_tilt = true; }
  if (fabs(zoom - 1.0f) >= 0.05) zoomed = 1;
  const int w = cols, h = rows;
  int wS1 = (int)(w * zoom), hS1 = (int)(h * zoom);
  double *H = P.H;
  if ((fabs(tilt - 1.) <= 0.1) && (fabs(phi) <= 0.2) && (fabs(zoom - 1.) <= 0.1)) {  // original image, :278-289
    const double E[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int i = 0; i < 9; i++) H[i] = E[i];
    P.identity = 1;
    P.ow = w; P.oh = h;
    return MODSX_OK;
  }
  P.identity = 0;
  double d, d2, w_new, h_new;
  double kV = 1., kH = 1.;
  if (zoomed) { kV = (double)w / (double)wS1; kH = (double)h / (double)hS1; }
  const bool q1 = (phi >= 0) && (phi < M_PI / 2);
  if (vertical_tilt) {
    if (q1) {
      w_new = floor((0.5 + cos(phi) * w + sin(phi) * h) / (kH));
      h_new = floor((0.5 + sin(phi) * w + cos(phi) * h) / (tilt * kV));
      H[0] = cos(phi) / kH; H[1] = sin(phi) / kH; H[2] = 0;
      H[3] = -sin(phi) / (tilt * kV); H[4] = cos(phi) / (tilt * kV); H[5] = floor(0.5 + sin(phi) * w / (tilt * kV));
    } else {
      w_new = floor((0.5 - cos(phi) * w + sin(phi) * h) / (kH));
      h_new = floor((0.5 + sin(phi) * w - cos(phi) * h) / (tilt * kV));
      d = -floor(cos(phi) * w / kH);
      d2 = floor(0.5 + (sin(phi) * w - cos(phi) * h) / (tilt * kV));
      H[0] = cos(phi) / kH; H[1] = sin(phi) / kH; H[2] = d;
      H[3] = -sin(phi) / (tilt * kV); H[4] = cos(phi) / (tilt * kV); H[5] = d2;
    }
  } else {
    if (q1) {
      w_new = floor((0.5 + cos(phi) * w + sin(phi) * h) / (tilt * kH));
      h_new = floor((0.5 + sin(phi) * w + cos(phi) * h) / (kV));
      H[0] = cos(phi) / (tilt * kH); H[1] = sin(phi) / (tilt * kH); H[2] = 0;
      H[3] = -sin(phi) / kV; H[4] = cos(phi) / kV; H[5] = floor(0.5 + sin(phi) * w / kV);
    } else {
      w_new = floor((0.5 - cos(phi) * w + sin(phi) * h) / (tilt * kH));
      h_new = floor((0.5 + sin(phi) * w - cos(phi) * h) / (kV));
      d = -floor(cos(phi) * w / (tilt * kH));
      d2 = floor(0.5 + (sin(phi) * w - cos(phi) * h) / kV);
      H[0] = cos(phi) / (tilt * kH); H[1] = sin(phi) / (tilt * kH); H[2] = d;
      H[3] = -sin(phi) / kV; H[4] = cos(phi) / kV; H[5] = d2;
    }
  }
  H[6] = 0; H[7] = 0; H[8] = 1;
  double sigma_aa_2 = zoomed ? InitSigma / (4.0 * zoom) : InitSigma / 2.0;
  double sigma_aa = InitSigma * tilt / (2.0 * zoom);
  double sigma_x = vertical_tilt ? sigma_aa_2 : sigma_aa, sigma_y = vertical_tilt ? sigma_aa : sigma_aa_2;
  double R[6];
  if (q1) {
    P.w_rot = floor((0.5 + cos(phi) * w + sin(phi) * h));
    P.h_rot = floor((0.5 + sin(phi) * w + cos(phi) * h));
    R[0] = cos(phi); R[1] = sin(phi); R[2] = 0;
    R[3] = -sin(phi); R[4] = cos(phi); R[5] = floor(0.5 + sin(phi) * w);
  } else {
    P.w_rot = floor((0.5 - cos(phi) * w + sin(phi) * h));
    P.h_rot = floor((0.5 + sin(phi) * w - cos(phi) * h));
    d = -floor(cos(phi) * w);
    d2 = floor(0.5 + (sin(phi) * w - cos(phi) * h));
    R[0] = cos(phi); R[1] = sin(phi); R[2] = d;
    R[3] = -sin(phi); R[4] = cos(phi); R[5] = d2;
  }
  P.ow = (int)w_new; P.oh = (int)h_new;
  if (P.w_rot <= 0 || P.h_rot <= 0 || P.ow <= 0 || P.oh <= 0) { set_error("degenerate synthesised view"); return MODSX_ERR_ARG; }
  invert_affine(R, P.Rinv);
  P.doBlur = v.doBlur;
  P.taps.clear();
  if (v.doBlur) {
    int kx = floor(2.0 * 3.0 * sigma_x + 1.0);
    if (kx % 2 == 0) kx++;
    if (kx < 3) kx = 3;
    int ky = floor(2.0 * 3.0 * sigma_y + 1.0);
    if (ky % 2 == 0) ky++;
    if (ky < 3) ky = 3;
    if (P.h_rot == 1) ky = 1;
    if (P.w_rot == 1) kx = 1;
    std::vector<float> KX = gaussian_kernel(kx, std::max(sigma_x, 0.));
    std::vector<float> KY = (ky == kx && fabs(sigma_x - sigma_y) < 2.220446049250313e-16) ? KX : gaussian_kernel(ky, std::max(sigma_y, 0.));
    P.kx = kx; P.ky = ky;
    P.taps = KX;
    P.taps.insert(P.taps.end(), KY.begin(), KY.end());
  }
  double Wz[6] = {0, 0, 0, 0, 0, 0};
  if (vertical_tilt) { Wz[0] = 1.0 / kH; Wz[4] = 1.0 / (tilt * kV); }
  else { Wz[0] = 1.0 / (tilt * kH); Wz[4] = 1.0 / kV; }
  invert_affine(Wz, P.Winv);
  return MODSX_OK;
}

int view_fused_kind(const ViewPlan &P, bool separate) {
  const double *W = P.Winv;
  int fused = P.doBlur && (P.kx >> 1) <= VF_RX && (P.ky >> 1) <= VF_RY;
  if (fused && !separate && W[1] == 0 && W[3] == 0 && W[0] > 0 && W[4] > 0) fused = 2;
  return fused;
}

static bool same_rotation(const ViewGroupIn &a, const ViewGroupIn &b) {
  return a.src == b.src && a.srows == b.srows && a.scols == b.scols && a.P->h_rot == b.P->h_rot && a.P->w_rot == b.P->w_rot &&
         memcmp(a.P->Rinv, b.P->Rinv, sizeof a.P->Rinv) == 0;
}

void group_views(const ViewGroupIn *v, int n, int cap, ViewGrouping &out) {
  out = ViewGrouping();
  out.group.assign(n, -1);
  out.order.reserve(n);
  std::vector<char> placed(n, 0);
  for (int i = 0; i < n; i++) {
    if (placed[i]) continue;
    placed[i] = 1;
    out.order.push_back(i);
    if (v[i].fused != 2) continue;
    const long long px = (long long)v[i].P->h_rot * v[i].P->w_rot;
    const long long tiles = (long long)((v[i].P->w_rot + VF_TW - 1) / VF_TW) * ((v[i].P->h_rot + VF_TH - 1) / VF_TH);
    const int g = out.nGroups++;
    int members = 1;
    out.group[i] = g;
    for (int k = i + 1; k < n && members < cap; k++) {
      if (placed[k] || v[k].fused != 2 || !same_rotation(v[i], v[k])) continue;
      placed[k] = 1;
      out.order.push_back(k);
      out.group[k] = g;
      members++;
    }
    out.nFused += members;
    out.tiles += tiles;
    out.rotPx += px;
    out.rotPxAlone += px * members;
  }
}

}  // namespace mx
