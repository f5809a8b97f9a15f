// Stand-alone run of the Hamming search's geometry and grouped table (mods_amd/csrc/kernels_hamming.hip: hamming_geometry,
// hamming_group_geometry) for the sanitizers: host code only, its own main, never loaded into Python, and no kernel is launched.
// It sweeps the grid of tests/test_reps_bin_cpu.py -- n1 in {1, 255, 256, 257, 5000}, nbytes in {1, 4, 5, 32, 33, 64}, G = 1..4,
// every partner size from {0, 2, T - 1, T, T + 1, 2 T + 3, 40 T} -- and checks every table against the single-problem cut.
// Build and run (from the repository root):
//   hipcc -O1 -g -std=c++17 -ffp-contract=off --offload-arch=gfx950 -x hip -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -I mods_amd/csrc -I include tests/native/hamming_group_check.cpp \
//         mods_amd/csrc/kernels_hamming.hip -o hamming_group_check && ./hamming_group_check
#include <cstdio>
#include <cstring>
#include "engine.hpp"

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { if (fails < 20) printf("FAILED line %d: %s (n1 %d nbytes %d)\n", __LINE__, #cond, g_n1, g_nb); fails++; } } while (0)
static int g_n1, g_nb;

static long check_group(int n1, const int *n2, int G, int nbytes) {
  using namespace mx;
  const int W = (nbytes + 3) / 4;
  HamGroup g;
  memset(&g, 0xab, sizeof g);                       // the function must set every field it hands to the kernels
  int prob[MATCH_MAXB] = {-1, -1, -1, -1};
  const int total = hamming_group_geometry(n1, n2, G, W, g, prob);
  CHECK(g.WK == hamming_kernel_width(W) && g.tile == 1024 / g.WK && g.gx == (n1 + 255) / 256);
  int p = 0, first = 0;
  for (int i = 0; i < G; i++) {
    if (n2[i] == 0) continue;
    const HammingGeo one = hamming_geometry(n1, n2[i], W, 0);
    CHECK(p < g.np && prob[p] == i);
    CHECK(g.n2[p] == n2[i] && g.ntiles[p] == one.ntiles && g.S[p] == one.S && g.tps[p] == one.tilesPerSplit && g.first[p] == first);
    CHECK(g.S[p] >= 1 && (g.S[p] - 1) * g.tps[p] < g.ntiles[p] && g.S[p] * g.tps[p] >= g.ntiles[p]);      // no empty split, all tiles
    CHECK((long)g.ntiles[p] * g.tile >= n2[i] && (long)(g.ntiles[p] - 1) * g.tile < n2[i]);
    // what the kernel computes for every split y of this problem: the problem found with three compares, a tile range inside it
    for (int s = 0; s < g.S[p]; s++) {
      const int y = first + s;
      const int found = (y >= g.first[1]) + (y >= g.first[2]) + (y >= g.first[3]);
      CHECK(found == p);
      const int t0 = (y - g.first[found]) * g.tps[found], t1 = t0 + g.tps[found] < g.ntiles[found] ? t0 + g.tps[found] : g.ntiles[found];
      CHECK(t0 >= 0 && t0 < t1 && t1 <= g.ntiles[found]);
      // the last row a tile load touches lies inside a stored buffer: its capacity is a multiple of 1024 rows >= n2
      CHECK((long)t1 * g.tile <= ((long)n2[i] + 1023) / 1024 * 1024);
    }
    first += g.S[p];
    p++;
  }
  CHECK(p == g.np && total == first);
  for (int k = g.np; k <= MATCH_MAXB; k++) CHECK(g.first[k] == total);
  return total;
}

int main() {
  const int N1[5] = {1, 255, 256, 257, 5000}, NB[6] = {1, 4, 5, 32, 33, 64};
  long tables = 0, splits = 0;
  for (int a = 0; a < 5; a++)
    for (int b = 0; b < 6; b++) {
      g_n1 = N1[a]; g_nb = NB[b];
      const int T = 1024 / mx::hamming_kernel_width((NB[b] + 3) / 4);
      const int sizes[7] = {0, 2, T - 1, T, T + 1, 2 * T + 3, 40 * T};
      for (int G = 1; G <= 4; G++) {
        int idx[4] = {0, 0, 0, 0};
        for (;;) {
          int n2[4];
          for (int i = 0; i < G; i++) n2[i] = sizes[idx[i]];
          splits += check_group(N1[a], n2, G, NB[b]);
          tables++;
          int i = 0;
          while (i < G && ++idx[i] == 7) idx[i++] = 0;
          if (i == G) break;
        }
      }
    }
  // the largest class: 2 000 000 rows on both sides, four partners
  const int big[4] = {2000000, 2000000, 2, 2000000};
  g_n1 = 2000000; g_nb = 64;
  splits += check_group(2000000, big, 4, 64);
  tables++;
  printf("%ld tables, %ld splits, %d failures\n", tables, splits, fails);
  return fails ? 1 : 0;
}
