// views_plan.hpp -- the host arithmetic of view synthesis (views_plan.cpp): the plan of one view (homography, sizes, the inverse
// maps of the two warps, the anti-alias taps), which launches it takes, and which views of a launch set share one rotation.  No
// HIP runtime call and no context: synth_views_batch (engine_views.hip) stages and launches what this plans,
// modsx_debug_view_plan / modsx_debug_views_groups (capi.hip) run it alone.
#pragma once
#include <vector>
#include "engine_api.hpp"

namespace mx {

// host half of GenerateSynthImageCorr (synth-detection.cpp:236-430) for one view: homography, sizes, the inverse maps of the
// two warps and the anti-alias taps
struct ViewPlan {
  int identity = 0;
  double H[9];
  int w_rot = 0, h_rot = 0, ow = 0, oh = 0, doBlur = 0, kx = 1, ky = 1;
  double Rinv[6], Winv[6];
  std::vector<float> taps;   // kx taps, then ky taps
};
int plan_view(int rows, int cols, const modsx_view &v, ViewPlan &P);

// Which launches a non-identity view takes: 2 = source image to tilted view in one launch (k_views_fused: a blur whose halo fits
// the tile, and a diagonal tilt / zoom map with positive scales: tap origins monotone in x and y, independent of the other),
// 1 = rotate + blur in one launch and the tilt in a second (the halo fits, the map is not diagonal, or `separate`), 0 = one
// launch per stage.
int view_fused_kind(const ViewPlan &P, bool separate);

// One non-identity view of a launch set as the grouping sees it: `src` only tells source images apart.
struct ViewGroupIn {
  const void *src;
  int srows, scols;
  const ViewPlan *P;
  int fused;            // view_fused_kind
};
// Views that take k_views_fused share a rotation when source image, source size, rotated size and the six doubles of Rinv match
// bit for bit: the rotated tile at a tile position is then the same f32 values for all of them, and one workgroup rotates it
// once.  A group takes at most `cap` views (a longer run of equal rotations is split), cap <= 1 makes every view its own group.
struct ViewGrouping {
  std::vector<int> order;     // the views in job-table order: a group's members next to each other, its first member where the
                              // view order has it; views that do not take the fused kernel where the view order has them
  std::vector<int> group;     // per view: its group, numbered in table order; -1 = does not take the fused kernel
  int nFused = 0, nGroups = 0;
  long long tiles = 0;        // VF_TW x VF_TH tiles of the fused launch: one grid of the rotated image per GROUP
  long long rotPx = 0;        // rotated pixels (w_rot x h_rot) per group, summed: what the fused launch rotates
  long long rotPxAlone = 0;   // ... and with every view a group of its own
};
void group_views(const ViewGroupIn *v, int n, int cap, ViewGrouping &out);

}  // namespace mx
