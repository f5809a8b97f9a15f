// engine_clahe.hip -- CLAHE on the device: what the reference's drivers do between imread and the first view when doCLAHE is set
// (mods.cpp:139-189, mods_multi.cpp:162-178, extract_features.cpp:92-103, export_descriptors.cpp:92-119: createCLAHE(),
// setClipLimit(4), apply on the 8-bit gray image).  The contract is CLAHE_Impl::apply of OpenCV 2.4.9, restated in
// include/modsx.h; the kernels are in kernels_clahe.hip.
//
// One call, or one batch of any number of images of any sizes, is three launches: a device table holds one ClaheImg per image,
// the grids' y axis is the image and their x axis is sized for the image that needs the most workgroups (the others' surplus
// workgroups leave at once).  Everything that depends on the image size alone -- tile and padded size, clipLimit (f64), lutScale
// (f32), the strip rule, the pixel pass's workgroups -- comes from clahe_geometry, which modsx_clahe_geometry reports unchanged.
//   strip rule   a histogram workgroup takes stripRows = max(1, CLAHE_STRIP_PX / tileW) whole rows of its tile, raised to
//                ceil(tileH / CLAHE_MAX_STRIPS) where a tile would be cut into more than CLAHE_MAX_STRIPS strips and never
//                more than tileH; strips = ceil(tileH / stripRows).  A 1024 x 768 image at 8 x 8 has 64 tiles of 128 x 96: 3 strips
//                each, 192 workgroups instead of 64.
//   pixel pass   ceil(rows * cols / CLAHE_APPLY_PX) workgroups, each over consecutive pixels in row-major order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <limits.h>
#include <string>
#include <unordered_set>
#include <vector>
#include "engine_api.hpp"

namespace mx {

int clahe_check(const char *fn, const modsx_clahe_params &p) {
  const std::string f(fn);
  if (p.tiles_x < 1 || p.tiles_y < 1) { set_error(f + ": tiles_x and tiles_y must be at least 1"); return MODSX_ERR_ARG; }
  if ((long long)p.tiles_x * p.tiles_y > CLAHE_MAX_TILES) {
    set_error(f + ": tiles_x * tiles_y above 256 (the LUT table of an image must fit 64 KiB of LDS)");
    return MODSX_ERR_ARG;
  }
  if (!(std::isfinite(p.clip_limit) && p.clip_limit >= 0)) { set_error(f + ": clip_limit must be finite and not negative"); return MODSX_ERR_ARG; }
  if (p.variant != 0 && p.variant != 1) { set_error(f + ": variant must be 0 (OpenCV 2.4.9) or 1 (OpenCV 3.x / 4.x)"); return MODSX_ERR_ARG; }
  return MODSX_OK;
}

int clahe_geometry(const char *fn, int rows, int cols, const modsx_clahe_params &p, ClaheGeo &g) {
  const int rc = clahe_check(fn, p);
  if (rc) return rc;
  if (rows < 1 || cols < 1 || rows > 16384 || cols > 16384 || (long long)rows * cols > (1ll << 26)) {
    set_error(std::string(fn) + ": image size outside 1 .. 16384 px per side / 64 Mpx");
    return MODSX_ERR_ARG;
  }
  const int tx = p.tiles_x, ty = p.tiles_y;
  if (cols % tx == 0 && rows % ty == 0) {
    g.padW = cols; g.padH = rows;
  } else {                   // both are padded, the divisible one by a whole grid: copyMakeBorder(.., ty - rows % ty, .., tx - cols % tx)
    g.padW = cols + (tx - cols % tx); g.padH = rows + (ty - rows % ty);
  }
  g.tileW = g.padW / tx; g.tileH = g.padH / ty;
  const int total = g.tileW * g.tileH;       // <= (16384 + 256)^2 / tiles, and 2^26 + a border for one tile: an int
  g.lutScale = (float)(CLAHE_BINS - 1) / total;
  g.clipLimit = 0;
  if (p.clip_limit > 0) {
    const double v = p.clip_limit * total / CLAHE_BINS;
    // a limit of `total` or more clips nothing, so the conversion of a huge product is capped instead of left undefined
    g.clipLimit = v >= (double)INT_MAX ? INT_MAX : (int)v;
    if (g.clipLimit < 1) g.clipLimit = 1;
  }
  g.stripRows = CLAHE_STRIP_PX / g.tileW;
  if (g.stripRows < 1) g.stripRows = 1;
  const int least = (g.tileH + CLAHE_MAX_STRIPS - 1) / CLAHE_MAX_STRIPS;
  if (g.stripRows < least) g.stripRows = least;
  if (g.stripRows > g.tileH) g.stripRows = g.tileH;
  g.strips = (g.tileH + g.stripRows - 1) / g.stripRows;
  g.applyBlocks = (int)(((long long)rows * cols + CLAHE_APPLY_PX - 1) / CLAHE_APPLY_PX);
  return MODSX_OK;
}

static int clahe_on_device(modsx_ctx *c, const char *fn, const float *p, const char *what) {
  hipPointerAttribute_t at;
  // the runtime answers for plain host memory too (as unregistered); only device and managed allocations are pixels a kernel may touch
  const bool known = hipPointerGetAttributes(&at, p) == hipSuccess;
  if (!known) (void)hipGetLastError();
  if (!known || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged)) {
    set_error(std::string(fn) + ": " + what + " does not hold device memory");
    return MODSX_ERR_ARG;
  }
  if (at.device != c->dev) { set_error(std::string(fn) + ": " + what + " lives on another device than the context"); return MODSX_ERR_ARG; }
  return MODSX_OK;
}

int clahe_batch(modsx_ctx *c, const char *fn, const modsx_image *const *in, modsx_image *const *out, int n, const modsx_clahe_params &p,
                int *dbgHist, unsigned char *dbgLut) {
  int rc = clahe_check(fn, p);
  if (rc) return rc;
  if (n == 0) return MODSX_OK;
  if (n > 65535) { set_error(std::string(fn) + ": more than 65535 images in one batch"); return MODSX_ERR_ARG; }
  const int tx = p.tiles_x, ty = p.tiles_y, tiles = tx * ty;
  std::vector<ClaheImg> tab(n);
  std::unordered_set<const float *> sources, targets;
  long long parts = 0, pixels = 0, strips = 0;
  int maxStrips = 1, maxBlocks = 1;
  for (int i = 0; i < n; i++) {
    const modsx_image *a = in[i];
    ClaheGeo g;
    if ((rc = clahe_geometry(fn, a->rows, a->cols, p, g))) return rc;
    if (out) {
      if (out[i]->rows != a->rows || out[i]->cols != a->cols) {
        set_error(std::string(fn) + ": the output image has another size than the input");
        return MODSX_ERR_ARG;
      }
      if ((rc = clahe_on_device(c, fn, out[i]->d, "the output image"))) return rc;
      if (!targets.insert(out[i]->d).second) { set_error(std::string(fn) + ": two outputs of a batch share their pixels"); return MODSX_ERR_ARG; }
    }
    if ((rc = clahe_on_device(c, fn, a->d, "the input image"))) return rc;
    sources.insert(a->d);
    ClaheImg &t = tab[i];
    t.src = a->d; t.dst = out ? out[i]->d : nullptr;
    t.partOfs = parts; t.lutOfs = (long long)i * tiles;
    t.rows = a->rows; t.cols = a->cols; t.tileW = g.tileW; t.tileH = g.tileH;
    t.strips = g.strips; t.stripRows = g.stripRows; t.clipLimit = g.clipLimit; t.applyBlocks = g.applyBlocks;
    t.lutScale = g.lutScale;
    t.vec = ((uintptr_t)t.src % 16 == 0 && (uintptr_t)t.dst % 16 == 0) ? 1 : 0;
    parts += (long long)tiles * g.strips;
    strips += (long long)tiles * g.strips;
    pixels += (long long)a->rows * a->cols;
    if (g.strips > maxStrips) maxStrips = g.strips;
    if (g.applyBlocks > maxBlocks) maxBlocks = g.applyBlocks;
  }
  // in place is one image's business; an output that another image of the batch reads would be written while it is read
  if (out)
    for (int i = 0; i < n; i++)
      if (out[i]->d != in[i]->d && sources.count(out[i]->d)) {
        set_error(std::string(fn) + ": an output of the batch is another image's input");
        return MODSX_ERR_ARG;
      }
  CtxBusy busy(c);
  const size_t tabBytes = sizeof(ClaheImg) * (size_t)n, lutBytes = (size_t)n * tiles * CLAHE_BINS;
  const size_t dbgBytes = dbgHist ? lutBytes * sizeof(int) : 0;
  if (!c->claheHost.ensure(tabBytes) || !c->claheTab.ensure(tabBytes) || !c->clahePart.ensure((size_t)parts * CLAHE_BINS * sizeof(int)) ||
      !c->claheLut.ensure(lutBytes) || (dbgBytes && !c->claheDbg.ensure(dbgBytes)))
    return MODSX_ERR_NOMEM;
  memcpy(c->claheHost.p, tab.data(), tabBytes);
  MX_HIP(hipMemcpyAsync(c->claheTab.p, c->claheHost.p, tabBytes, hipMemcpyHostToDevice, c->stream));
  const ClaheImg *dtab = (const ClaheImg *)c->claheTab.p;
  hipEvent_t ev[4];
  const bool timed = c->prof.enabled;     // modsx_profile: the launches are timed into the context (tools/bench_clahe.py), no new kernel class
  if (timed) for (int i = 0; i < 4; i++) MX_HIP(hipEventCreate(&ev[i]));
  if (timed) hipEventRecord(ev[0], c->stream);
  launch_clahe_hist(c->stream, dtab, n, tx, ty, maxStrips, (int *)c->clahePart.p);
  if (timed) hipEventRecord(ev[1], c->stream);
  launch_clahe_lut(c->stream, dtab, n, tiles, p.variant, (const int *)c->clahePart.p, (unsigned char *)c->claheLut.p,
                   dbgHist ? (int *)c->claheDbg.p : nullptr);
  if (timed) hipEventRecord(ev[2], c->stream);
  if (out) launch_clahe_apply(c->stream, dtab, n, tx, ty, p.variant, maxBlocks, (const unsigned char *)c->claheLut.p);
  if (timed) hipEventRecord(ev[3], c->stream);
  hipError_t e = hipSuccess;
  if (dbgHist) e = hipMemcpyAsync(dbgHist, c->claheDbg.p, dbgBytes, hipMemcpyDeviceToHost, c->stream);
  if (dbgLut && e == hipSuccess) e = hipMemcpyAsync(dbgLut, c->claheLut.p, lutBytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipGetLastError();
  if (timed) {
    float ms[3] = {0, 0, 0};
    bool ok = e == hipSuccess;
    for (int i = 0; i < 3 && ok; i++) ok = hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]) == hipSuccess;
    if (ok) for (int i = 0; i < 3; i++) c->claheMs[i] = ms[i];
    for (int i = 0; i < 4; i++) hipEventDestroy(ev[i]);
  }
  MX_HIP(e);
  c->claheCounters[0]++;
  c->claheCounters[1] += n;
  c->claheCounters[2] += (long)n * tiles;
  c->claheCounters[3] += (long)strips;
  c->claheCounters[4] += (long)pixels;
  c->claheCounters[5] += out ? 3 : 2;
  return MODSX_OK;
}

}  // namespace mx
