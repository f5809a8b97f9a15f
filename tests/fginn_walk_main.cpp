// Stand-alone run of mods_amd/csrc/fginn_walk.hpp (tests/test_fginn_walk_cpu.py builds it with the host compiler, plain and under
// -fsanitize=address,undefined, and runs it as a child under a time limit).  Only the header and the standard library.
//
// argv[1] is a case file of whitespace-separated hexadecimal words, any number of runs one after the other:
//   np n1 nn ratio cd                       ratio, cd: the bit patterns of two f64; every problem of a run shares them and n1
//   per problem: n2, pos2 [n2][2] as f64 bit patterns, then per query its n2 neighbour keys, sorted
// The first four keys of a query are its top4 (all ones where n2 < 4); the problems' open steps fill one open list (pad = the
// problem).  k_f32_resolve is then played on the host from its definition in kernels_fginn32.hip: among the keys > klast a train
// is terminal when d >= dpass or it lies farther than cd from train t0 (f64); kterm = the smallest terminal key, cnt = the count of
// the others.  After the close step the program prints, per run, "run <np> <n1> <open entries> <closed by count>" and per problem
// "problem <p> <records>", a line "q t0 tj t1 d1 d2 d2by2ndcl ratio" per record (the f64 as bit patterns) and "stages" with a digit
// per query.
#include <cstdio>
#include <cstdlib>
#include "../mods_amd/csrc/fginn_walk.hpp"

using namespace mx;
typedef unsigned long long u64;

static bool word(FILE *f, u64 *v) { return fscanf(f, "%llx", v) == 1; }
static u64 need(FILE *f) {
  u64 v;
  if (!word(f, &v)) { fprintf(stderr, "case file ends inside a run\n"); exit(2); }
  return v;
}
static double f64_of(u64 b) { double d; memcpy(&d, &b, 8); return d; }
static u64 bits_of(double d) { u64 b; memcpy(&b, &d, 8); return b; }

struct Problem {
  int n2;
  std::vector<double> pos;      // [n2][2]
  std::vector<u64> keys;        // [n1][n2]
};

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: fginn_walk_main <case file>\n"); return 2; }
  FILE *f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  u64 first;
  while (word(f, &first)) {
    const int np = (int)first, n1 = (int)need(f), nn = (int)need(f);
    const double ratio = f64_of(need(f)), cd = f64_of(need(f));
    const double rsq = ratio * ratio, cd2 = cd * cd;
    std::vector<Problem> prob(np);
    std::vector<u64> top4((size_t)np * n1 * 4, KEY_NONE);
    for (int p = 0; p < np; p++) {
      Problem &P = prob[p];
      P.n2 = (int)need(f);
      P.pos.resize((size_t)P.n2 * 2);
      for (double &v : P.pos) v = f64_of(need(f));
      P.keys.resize((size_t)n1 * P.n2);
      for (u64 &k : P.keys) k = need(f);
      for (int q = 0; q < n1; q++)
        for (int j = 0; j < 4 && j < P.n2; j++) top4[((size_t)p * n1 + q) * 4 + j] = P.keys[(size_t)q * P.n2 + j];
    }

    std::vector<FginnWalk> walks(np);
    std::vector<F32Open> open;
    for (int p = 0; p < np; p++)
      fginn_walk_open(top4.data() + (size_t)p * n1 * 4, n1, prob[p].pos.data(), rsq, cd2, nn, p, walks[p], open);

    std::vector<F32Closed> closed(open.size(), F32Closed{KEY_NONE, 0u, 0u});
    for (size_t u = 0; u < open.size(); u++) {
      const F32Open &o = open[u];
      const Problem &P = prob[o.pad];
      const double px = P.pos[2 * (size_t)o.t0], py = P.pos[2 * (size_t)o.t0 + 1];
      for (int j = 0; j < P.n2; j++) {
        const u64 key = P.keys[(size_t)o.q * P.n2 + j];
        if (!(key > o.klast)) continue;
        const int idx = key_idx(key);
        const double dx = px - P.pos[2 * (size_t)idx], dy = py - P.pos[2 * (size_t)idx + 1];
        if (key_dist(key) >= o.dpass || dx * dx + dy * dy > cd2) closed[u].kterm = std::min(closed[u].kterm, key);
        else closed[u].cnt++;
      }
    }
    const int byCount = fginn_walk_close(open, closed.data(), top4.data(), n1, rsq, nn, walks.data());

    printf("run %d %d %zu %d\n", np, n1, open.size(), byCount);
    for (int p = 0; p < np; p++) {
      std::vector<modsx_tentative> out;
      fginn_walk_emit(walks[p], out);
      printf("problem %d %zu\n", p, out.size());
      for (const modsx_tentative &t : out)
        printf("%d %d %d %d %llx %llx %llx %llx\n", t.q, t.t0, t.tj, t.t1, bits_of(t.d1), bits_of(t.d2), bits_of(t.d2by2ndcl), bits_of(t.ratio));
      printf("stages ");
      for (int q = 0; q < n1; q++) putchar('0' + walks[p].stage[q]);
      putchar('\n');
    }
  }
  fclose(f);
  return 0;
}
