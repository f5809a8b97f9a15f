// engine_patchdesc.hip -- the driver of the descriptors that are one kernel per normalised 41 x 41 patch (LIOP, SURF, DAISY:
// engine_liop.hip, engine_surf.hip, engine_daisy.hip give it a PatchDesc).
//   * caller-supplied patches: device rows are read in place with one launch; host rows pass through the context's patch buffer
//     (patchBuf, at most 64 MiB) in sub-batches, copy then launch, output rows at out + j0 * dim;
//   * regions: the description front end unchanged (describe_batch_tail), with the patch-out form of k_describe into patchBuf and
//     then the descriptor's kernel as the last launches of a chunk, in sub-batches of the chunk's jobs;
//   * a sub-batch holds what fits 64 MiB, or what the descriptor's environment variable says (1 .. that many, read once per process);
//   * rows on their way to a host caller are staged in patchOut.  Calls on a context are serialised (CtxBusy) and each copies its
//     rows out before it returns, so one patch buffer and one staging buffer serve every descriptor.
// Both entries only enqueue: the caller adds what it still wants on the stream, then patch_sync, its counters and patch_fetch.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include "engine_api.hpp"

namespace mx {

constexpr int PATCH_NPX = 41 * 41;
constexpr size_t PATCH_B = (size_t)PATCH_NPX * 4, PATCH_BUF_B = (size_t)64 << 20;

// patches per sub-batch: what fits 64 MiB, or the value of `env` (1 .. that many); each name is read once per process
static int sub_batch(const char *env) {
  static std::mutex mu;
  static std::map<std::string, int> seen;
  std::lock_guard<std::mutex> lock(mu);
  auto it = seen.find(env);
  if (it == seen.end()) {
    const long full = (long)(PATCH_BUF_B / PATCH_B);
    const char *e = getenv(env);
    const long v = e ? atol(e) : full;
    it = seen.emplace(env, (int)std::min(std::max(v, 1L), full)).first;
  }
  return it->second;
}

int patchdesc_patches(modsx_ctx *c, const PatchDesc &d, const float *patches, int n, float *desc, bool onDevice, long *subBatches) {
  if (onDevice) {
    // rows that already live in HBM are read where they are
    d.launch(d.self, c->stream, patches, n, 0, desc, nullptr);
    *subBatches = 1;
    return MODSX_OK;
  }
  const int B = std::min(sub_batch(d.batchEnv), n);
  if (!c->patchBuf.ensure((size_t)B * PATCH_B) || !c->patchOut.ensure((size_t)n * d.dim * 4)) return MODSX_ERR_NOMEM;
  for (int j0 = 0; j0 < n; j0 += B, ++*subBatches) {
    const int nb = std::min(B, n - j0);
    MX_HIP(hipMemcpyAsync(c->patchBuf.p, patches + (size_t)j0 * PATCH_NPX, (size_t)nb * PATCH_B, hipMemcpyHostToDevice, c->stream));
    d.launch(d.self, c->stream, (const float *)c->patchBuf.p, nb, j0, (float *)c->patchOut.p + (size_t)j0 * d.dim, nullptr);
  }
  return MODSX_OK;
}

struct PatchTail { const PatchDesc *d; float *out; int first; long *subBatches; };
static int tail_patchdesc(modsx_ctx *c, void *self, const DescJob *jobs, int n, const float *grid, const int *needTab,
                          const float *coordTab, int photoNorm) {
  PatchTail *t = (PatchTail *)self;
  const int B = std::min(sub_batch(t->d->batchEnv), n);
  if (!c->patchBuf.ensure((size_t)B * PATCH_B)) return MODSX_ERR_NOMEM;
  // the launches of a stream run in order: sub-batch k + 1 overwrites the buffer after the descriptor's kernel of sub-batch k has
  // read it.  The jobs carry their output rows, so every sub-batch gets the output base
  for (int j0 = 0; j0 < n; j0 += B, ++*t->subBatches) {
    const int nb = std::min(B, n - j0);
    launch_describe_patch(c->stream, jobs + j0, nb, (const ImgRef *)c->imgRefs.p, grid, needTab, coordTab, c->dSiftMaskIdx, c->nSiftMask,
                          photoNorm, (float *)c->patchBuf.p, 0);
    t->d->launch(t->d->self, c->stream, (const float *)c->patchBuf.p, nb, t->first + j0, t->out, jobs + j0);
  }
  t->first += n;
  return MODSX_OK;
}

int patchdesc_regions(modsx_ctx *c, const PatchDesc &d, const modsx_image *img, const modsx_region *regs, int n, double mrSize,
                      int patchSize, int fast, int photoNorm, float *desc, bool onDevice, long *subBatches) {
  PatchTail t = {&d, desc, 0, subBatches};
  if (!onDevice) { if (!c->patchOut.ensure((size_t)n * d.dim * 4)) return MODSX_ERR_NOMEM; t.out = (float *)c->patchOut.p; }
  const std::vector<modsx_region> v(regs, regs + n);
  const DescTail tail = {tail_patchdesc, &t};
  return describe_batch_tail(c, img, v, mrSize, patchSize, fast, photoNorm, tail);
}

int patch_sync(modsx_ctx *c) {
  MX_HIP(hipStreamSynchronize(c->stream));
  MX_HIP(hipGetLastError());
  return MODSX_OK;
}

int patch_fetch(modsx_ctx *c, float *rows, size_t floats, bool onDevice) {
  if (!onDevice) MX_HIP(hipMemcpy(rows, c->patchOut.p, floats * 4, hipMemcpyDeviceToHost));
  return MODSX_OK;
}

}  // namespace mx
