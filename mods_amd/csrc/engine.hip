// engine.hip -- host orchestration of the device path (C++ above HIP, below the C ABI): context, waits, copies, profiler,
// then orientation, description, matching and verification.  The detection front end (pyramid, extrema, detection order, affine
// adaptation) is in engine_detect.hip.
//
// Mirrors, stage by stage, what the reference does per synthesised view in
// ImageRepresentation::SynthDetectDescribeKeypoints (imagerepresentation.cpp:603-2047) and per pair
// in mods.cpp:229-415.  Dense per-pixel / per-patch work runs in the HIP kernels; the host keeps the
// order-dependent bookkeeping (detection order, first-come octaveMap claims, std::sort) and the few
// libm transcendentals (powf / cos / sin / exp) so they are evaluated by the same libm as on the CPU path.
#include <atomic>
#include <math.h>
#include <stdio.h>
#include <algorithm>
#include <chrono>
#include <map>
#include <unordered_set>
#include <mutex>
#include <string>
#include "engine_api.hpp"
#include "describe_plan.hpp"

#ifdef MODSX_DUP_BUILD
namespace mx {
int dup_count(int cls) {
  static const long mask = getenv("MODSX_DUP") ? strtol(getenv("MODSX_DUP"), nullptr, 0) : 0;
  return 1 + (int)((mask >> cls) & 1);
}
}  // namespace mx
#endif
namespace mx {

static thread_local std::string g_err;
void set_error(const std::string &s) { g_err = s; }
static std::atomic<int> g_busyContexts{0};
bool gpu_shared() { return g_busyContexts.load(std::memory_order_relaxed) > 1; }
CtxBusy::CtxBusy(modsx_ctx *ctx) : c(ctx) {
  if (c && c->busyDepth++ == 0) {
    g_busyContexts.fetch_add(1, std::memory_order_relaxed);
    // how this call waits at its stage boundaries is decided once, here (MODSX_HOST_WAIT=auto follows the process' CPU load): a
    // context that goes back from the flag word to the runtime's wait first lets the runtime catch up with its stream -- the
    // runtime has not been asked about that stream since the context left its wait, and the small copies it does with the CPU
    // (rocprofv3 run of the 16-stream bench: SIGSEGV inside hipMemcpyAsync) rest on its own picture of what has completed
    const bool rt = host_wait_runtime() || !c->hFlag;
    if (rt && !c->waitRuntime) hipStreamSynchronize(c->stream);
    c->waitRuntime = rt;
  }
}
CtxBusy::~CtxBusy() { if (c && --c->busyDepth == 0) g_busyContexts.fetch_sub(1, std::memory_order_relaxed); }
const char *last_error() { return g_err.c_str(); }

bool DevBuf::ensure(size_t bytes) {
  if (bytes <= cap) return true;
  release();
  size_t want = bytes + bytes / 4 + 256;
  if (hipMalloc(&p, want) != hipSuccess) { p = nullptr; cap = 0; set_error("hipMalloc failed"); return false; }
  cap = want;
  return true;
}
void DevBuf::release() { if (p) hipFree(p); p = nullptr; cap = 0; }
bool PinBuf::ensure(size_t bytes) {
  if (bytes <= cap) return true;
  release();
  size_t want = bytes + bytes / 4 + 256;
  if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { p = nullptr; cap = 0; set_error("hipHostMalloc failed"); return false; }
  cap = want;
  return true;
}
void PinBuf::release() { if (p) hipHostFree(p); p = nullptr; cap = 0; }

// ---- stage boundaries without the runtime's wait machinery -------------------------------------------------------------------------
// What a stage boundary costs the HOST was measured in isolation (tools/ubench/host_sync.hip, 16 threads with a stream each, 8
// kernels + results + wait per iteration, waits of ~3 ms): with hipMemcpyAsync + hipStreamSynchronize 500 us of CPU per
// iteration (340 in the caller: the runtime watches the signal for 200 us before it sleeps in the kernel driver, and 160 in the
// runtime's own threads), 3 ms when an H2D hipMemcpyAsync is part of the iteration (the wait then spins to the end) -- against
// 73 us when the last kernel writes a sequence word into pinned memory and the thread looks at it between naps.  So the hot path
// neither copies nor waits through the runtime:
//   ctx_copy   device <-> PINNED host memory by a kernel on the context's stream (system-scope accesses on the host side);
//   ctx_sync   a one-lane kernel writes the context's next sequence number to its pinned flag word behind everything issued so
//              far; the thread spins for a few microseconds, then naps (10 us growing to 100 us, timer slack 2 us) until it
//              sees it.  After 20 s without it hipStreamSynchronize is asked (a faulted queue never writes the flag).
// In the pipeline the gain is smaller than in isolation (host_wait_runtime below says when it is taken): most of a pair's host CPU
// is the engine's own loops in the context threads (19-20 of 25 ms), not the waits.
}  // namespace mx
#include <sys/prctl.h>
#include <time.h>
namespace mx {
__global__ void k_flag(unsigned *flag, unsigned seq) {
  __threadfence_system();
  __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// HOST_SRC: the source is pinned host memory -- a system-scope acquire in front of the loads drops whatever an earlier launch left
// in the caches of those addresses; otherwise the destination is, and a system-scope release follows the stores.  16 bytes per lane
// (1 KB per wave instruction: the PCIe link sees whole cache lines; 8-byte system-scope atomics per lane moved a 2 MB table at a
// fifth of the rate and cost the pipeline 10 %).
template <bool HOST_SRC>
__global__ __launch_bounds__(256) void k_copy_pinned(uint4 *dst, const uint4 *src, size_t n16, int tail) {
  if (HOST_SRC) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
  const size_t stride = (size_t)gridDim.x * 256;
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < n16; i += 4 * stride) {
    const uint4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
    dst[i] = a; dst[i + stride] = b; dst[i + 2 * stride] = c; dst[i + 3 * stride] = d;
  }
  for (; i < n16; i += stride) dst[i] = src[i];
  if (tail && blockIdx.x == 0 && threadIdx.x < (unsigned)tail)
    reinterpret_cast<unsigned char *>(dst + n16)[threadIdx.x] = reinterpret_cast<const unsigned char *>(src + n16)[threadIdx.x];
  if (!HOST_SRC) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
}
// MODSX_HOST_WAIT = runtime | flag | auto (default).  Measured (16 contexts, one GPU, 16 CPUs): on the headline workload, which uses a
// third of the CPUs, the flag wait takes 0.0255 -> 0.0215 CPU-s per pair (the runtime's own threads 4.7 -> 2.1 ms, system time
// 3.7 -> 1.7 ms) and costs 1.2 % of the pairs/s (the naps wake tens of microseconds late at ~30 boundaries per pair); on the cviu
// ladder, whose MSER steps keep all 16 CPUs busy, it takes 0.244 -> 0.206 CPU-s per pair and GIVES 13 % (61.7 -> 70.0 pairs/s).
// So `auto` looks at what the process is short of: every 50 ms it compares the CPU time the process used with its allowance
// (cgroup quota / local ranks) -- above 80 % the host is the limit and the flag wait is taken, below 60 % the runtime's wait.
}  // namespace mx
#include <sys/resource.h>
namespace mx {
bool host_wait_runtime() {
  static const int forced = [] {
    const char *e = getenv("MODSX_HOST_WAIT");
    if (e && !strcmp(e, "runtime")) return 1;
    if (e && !strcmp(e, "flag")) return 0;
    if (e && !strcmp(e, "alternate")) return 2;      // test aid: every call of this function answers the other way (the transitions)
    return -1;
  }();
  if (forced == 2) { static std::atomic<unsigned> flip{0}; return (flip.fetch_add(1, std::memory_order_relaxed) & 1) != 0; }
  if (forced >= 0) return forced != 0;
  static const double allowance = (double)host_cpus_per_rank();
  static std::atomic<int> rt{allowance >= 8 ? 1 : 0};
  static std::atomic<long long> nextNs{0};
  static std::atomic<long long> lastWallNs{0}, lastCpuUs{0};
  const long long now = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
  long long due = nextNs.load(std::memory_order_relaxed);
  if (now >= due && nextNs.compare_exchange_strong(due, now + 50000000LL, std::memory_order_relaxed)) {     // one thread per period
    rusage ru;
    getrusage(RUSAGE_SELF, &ru);
    const long long cpu = (ru.ru_utime.tv_sec + ru.ru_stime.tv_sec) * 1000000LL + ru.ru_utime.tv_usec + ru.ru_stime.tv_usec;
    const long long w0 = lastWallNs.exchange(now), c0 = lastCpuUs.exchange(cpu);
    if (w0 && now - w0 < 1000000000LL) {           // (a longer gap: the process was idle in between, the figure says nothing)
      const double load = (double)(cpu - c0) * 1e3 / (double)(now - w0) / allowance;
      if (load > 0.80) rt.store(0, std::memory_order_relaxed);
      else if (load < 0.60) rt.store(1, std::memory_order_relaxed);
    }
  }
  return rt.load(std::memory_order_relaxed) != 0;
}
hipError_t ctx_copy(modsx_ctx *c, void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
  if (!bytes) return hipSuccess;
  const bool h2d = kind == hipMemcpyHostToDevice;
  static const bool rtCopy = [] { const char *e = getenv("MODSX_HOST_COPY"); return e && !strcmp(e, "runtime"); }();
  // tables above 64 KB stay with the runtime's copy engines: as kernels on the stream they cost the pipeline 3 % (the describe
  // blobs and candidate lists are megabytes; a copy kernel holds the stream for tens of microseconds that the DMA engine overlaps)
  static const size_t rtAbove = getenv("MODSX_HOST_COPY_MAX") ? (size_t)atol(getenv("MODSX_HOST_COPY_MAX")) : 65536;
  if (c->waitRuntime || rtCopy || bytes > rtAbove || (!h2d && kind != hipMemcpyDeviceToHost) || (((uintptr_t)dst | (uintptr_t)src) & 15))
    return hipMemcpyAsync(dst, src, bytes, kind, c->stream);
  const size_t n16 = bytes >> 4;
  const int tail = (int)(bytes & 15);
  const unsigned grid = (unsigned)std::min<size_t>(std::max<size_t>((n16 + 1023) / 1024, 1), 512);
  if (h2d) hipLaunchKernelGGL(k_copy_pinned<true>, dim3(grid), dim3(256), 0, c->stream, (uint4 *)dst, (const uint4 *)src, n16, tail);
  else hipLaunchKernelGGL(k_copy_pinned<false>, dim3(grid), dim3(256), 0, c->stream, (uint4 *)dst, (const uint4 *)src, n16, tail);
  return hipGetLastError();
}
unsigned ctx_mark(modsx_ctx *c) {
  const unsigned seq = ++c->flagSeq;
  hipLaunchKernelGGL(k_flag, dim3(1), dim3(1), 0, c->stream, c->hFlag, seq);
  return seq;
}
bool ctx_mark_reached(modsx_ctx *c, unsigned seq) {
  return (int)(__atomic_load_n(c->hFlag, __ATOMIC_ACQUIRE) - seq) >= 0;
}
hipError_t ctx_wait_mark(modsx_ctx *c, unsigned seq) {
  static const int spinUs = getenv("MODSX_WAIT_SPIN_US") ? atoi(getenv("MODSX_WAIT_SPIN_US")) : 6;
  static const long napMax = getenv("MODSX_WAIT_NAP_MAX_US") ? atol(getenv("MODSX_WAIT_NAP_MAX_US")) * 1000 : 100000;
  if (ctx_mark_reached(c, seq)) return hipSuccess;
  const auto t0 = std::chrono::steady_clock::now();
  auto us_since = [&]() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); };
  for (int i = 0;; i++) {
    if (ctx_mark_reached(c, seq)) return hipSuccess;
    __builtin_ia32_pause();
    if ((i & 15) == 15 && us_since() >= spinUs) break;
  }
  static thread_local bool slack = false;
  if (!slack) { prctl(PR_SET_TIMERSLACK, 2000UL, 0, 0, 0); slack = true; }   // the naps below mean what they say (default slack: 50 us)
  // naps of 10 us growing to 100: 20-30 looks at a wait of 1-3 ms.  (Tried: one long nap sized from the last waits at the same call
  // site, then close looks -- under 16 streams a stage's wait varies too much, the thread woke late and the pairs/s fell by 3 %;
  // naps of 5 us throughout: the runtime's throughput for more CPU than the runtime's own wait takes.)
  long nap = std::min(10000L, napMax);
  for (int k = 0;; k++) {
    timespec ts = {0, nap};
    nanosleep(&ts, nullptr);
    if (ctx_mark_reached(c, seq)) return hipSuccess;
    if ((k & 1) && nap < napMax) nap = std::min(nap * 2, napMax);
    if ((k & 255) == 255 && us_since() > 20e6) break;
  }
  const hipError_t e = hipStreamSynchronize(c->stream);     // a queue that faulted never writes the flag: let the runtime say what happened
  if (e == hipSuccess && !ctx_mark_reached(c, seq)) return hipErrorUnknown;
  return e;
}
hipError_t ctx_sync(modsx_ctx *c) {
  if (c->waitRuntime || !c->hFlag) return hipStreamSynchronize(c->stream);
  const unsigned seq = ctx_mark(c);
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) return le;
  return ctx_wait_mark(c, seq);
}

// ---- per-kernel-class GPU timing with HIP events on the launch stream ------------------------------
// the next slot of the profiler, its two events created on first use
static size_t prof_take_slot(Profiler &p, int cls, double work) {
  if (p.used == p.evA.size()) {
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    p.evA.push_back(a); p.evB.push_back(b); p.cls.push_back(0);
  }
  const size_t slot = p.used++;
  p.cls[slot] = cls;
  p.work[cls] += work;
  p.launches[cls]++;
  return slot;
}
void prof_begin(modsx_ctx *c, int cls, double work, size_t *slot) {
  *slot = (size_t)-1;
  if (!c->prof.enabled) return;
  *slot = prof_take_slot(c->prof, cls, work);
  hipEventRecord(c->prof.evA[*slot], c->stream);
}
void prof_end(modsx_ctx *c, size_t slot) { if (slot != (size_t)-1) hipEventRecord(c->prof.evB[slot], c->stream); }
// a slot whose two events the caller records itself (around one launch inside a launch helper); false when profiling is off
bool prof_reserve(modsx_ctx *c, int cls, double work, hipEvent_t *ev2) {
  if (!c->prof.enabled) return false;
  const size_t slot = prof_take_slot(c->prof, cls, work);
  ev2[0] = c->prof.evA[slot]; ev2[1] = c->prof.evB[slot];
  return true;
}
void prof_collect(modsx_ctx *c) {
  Profiler &p = c->prof;
  if (!p.enabled || !p.used) return;
  hipStreamSynchronize(c->stream);
  for (size_t i = 0; i < p.used; i++) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, p.evA[i], p.evB[i]) == hipSuccess) p.ms[p.cls[i]] += ms;
  }
  p.used = 0;
}
void prof_reset(modsx_ctx *c, bool enable) {
  Profiler &p = c->prof;
  p.enabled = enable; p.used = 0;
  for (int i = 0; i < K_NCLASS; i++) { p.ms[i] = 0; p.work[i] = 0; p.launches[i] = 0; }
}

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
// The tables of k_orientation, on the host: the voting list and the bin table (one copy: upload_tables sends them to the device,
// modsx_orientation_tables shows them)
int orientation_tables_host(OriTables &t) {
  const int PS = 41, PSP = ORI_PSP;
  std::vector<float> m(PS * PS);
  circular_gauss_mask(m.data(), PS, PS / 3.0f);  // EstimateDominantAnglesFunctor ctor, synth-detection.cpp:757-762
  // the pixels that can vote (mask > 0; all lie inside the 1-pixel frame the gradient needs), raster order, as indices
  // into k_orientation's 44-column patch
  std::vector<unsigned short> &idx = t.idxRaster;
  std::vector<float> &w = t.wRaster;
  idx.clear(); w.clear();
  for (int r = 1; r < PS - 1; r++)
    for (int q = 1; q < PS - 1; q++)
      if (m[r * PS + q] > 0) { idx.push_back((unsigned short)(r * PSP + q)); w.push_back(m[r * PS + q]); }
  for (int r = 0; r < PS; r++)
    for (int q = 0; q < PS; q++)
      if ((r == 0 || q == 0 || r == PS - 1 || q == PS - 1) && m[r * PS + q] > 0) {
        set_error("orientation mask reaches the patch frame");
        return MODSX_ERR_ARG;
      }
  if ((int)idx.size() > ORI_NV) { set_error("orientation voting list exceeds ORI_NV"); return MODSX_ERR_ARG; }
  t.nReal = (int)idx.size();
  while ((int)idx.size() < ORI_NV) { idx.push_back((unsigned short)(PSP + 1)); w.push_back(0.f); }
  {   // k_orientation's lane l takes the CONTIGUOUS list elements [PER_L l, PER_L (l + 1)) and reads table entry lane + 64 q
    constexpr int PER_L = ORI_NV / 64;
    t.idxLanes.assign(ORI_NV, 0);
    t.wLanes.assign(ORI_NV, 0.f);
    for (int l = 0; l < 64; l++)
      for (int q = 0; q < PER_L; q++) { t.idxLanes[l + 64 * q] = idx[PER_L * l + q]; t.wLanes[l + 64 * q] = w[PER_L * l + q]; }
  }
  // the histogram bin is a function of atan2LUTff's angle, which takes 8 x 256 values (kmath.hpp: atan2lut_case / _value) and
  // 0 in the special case (entry 2048): tabulated with the kernel's own expression
  t.binTab.assign(ATAN_CASES, 0);
  const double *L = atan_lut_host();
  const float PIf = float(M_PI);
  for (int e = 0; e < ATAN_CASES; e++) {
    const float ori = e < 2048 ? atan2lut_value(L, e >> 8, e & 255) : 0.f;
    t.binTab[e] = (unsigned char)(int)(36 * (ori / PIf + 1.0f) / 2.0f);          // synth-detection.cpp:781-786 as in k_orientation
  }
  return MODSX_OK;
}

static int upload_tables(modsx_ctx *c) {
  const int PS = 41;
  std::vector<float> m(PS * PS);
  OriTables ot;
  {
    const int rc = orientation_tables_host(ot);
    if (rc != MODSX_OK) return rc;
    MX_HIP(hipMalloc(&c->dOriMask, ORI_NV * 4));
    MX_HIP(hipMalloc(&c->dOriIdx, ORI_NV * 2));
    MX_HIP(hipMemcpy(c->dOriMask, ot.wLanes.data(), ORI_NV * 4, hipMemcpyHostToDevice));
    MX_HIP(hipMemcpy(c->dOriIdx, ot.idxLanes.data(), ORI_NV * 2, hipMemcpyHostToDevice));
  }
  MX_HIP(hipMalloc(&c->dSiftMask, PS * PS * 4));
  circular_gauss_mask(m.data(), PS, 0);          // SIFTDescriptor ctor / DescribeRegions, siftdesc.h:87
  MX_HIP(hipMemcpy(c->dSiftMask, m.data(), PS * PS * 4, hipMemcpyHostToDevice));
  {
    std::vector<unsigned short> idx;
    for (int i = 0; i < PS * PS; i++) if (m[i] > 0) idx.push_back((unsigned short)i);
    c->nSiftMask = (int)idx.size();
    MX_HIP(hipMalloc(&c->dSiftMaskIdx, idx.size() * 2));
    MX_HIP(hipMemcpy(c->dSiftMaskIdx, idx.data(), idx.size() * 2, hipMemcpyHostToDevice));
  }
  MX_HIP(hipMalloc(&c->dAtan, 256 * 8));
  MX_HIP(hipMemcpy(c->dAtan, atan_lut_host(), 256 * 8, hipMemcpyHostToDevice));
  {
    // What the gradient stages need of atan2LUTff's angle is a function of it: the histogram bin (orientation:
    // orientation_tables_host) and the fractional SIFT orientation bin (description).  The angle takes 8 x 256 values (kmath.hpp:
    // atan2lut_case / _value) and 0 in the special case (entry 2048), so both functions are tabulated with the kernels' own expressions.
    std::vector<float> so(ATAN_CASES);
    const double *L = atan_lut_host();
    const double TWO_PI = 6.28318530718;
    for (int e = 0; e < ATAN_CASES; e++) {
      const float ori = e < 2048 ? atan2lut_value(L, e >> 8, e & 255) : 0.f;
      so[e] = (float)((double)8.0f * ((double)ori + TWO_PI) / TWO_PI);         // siftdesc.cpp:103-110 as in k_describe
    }
    MX_HIP(hipMalloc(&c->dOriBinTab, ATAN_CASES));
    MX_HIP(hipMemcpy(c->dOriBinTab, ot.binTab.data(), ATAN_CASES, hipMemcpyHostToDevice));
    MX_HIP(hipMalloc(&c->dSiftOTab, ATAN_CASES * 4));
    MX_HIP(hipMemcpy(c->dSiftOTab, so.data(), ATAN_CASES * 4, hipMemcpyHostToDevice));
  }
  // precomputeBinsAndWeights, matching/siftdesc.cpp:22-71 (spatialBins 4, orientationBins 8, patch 41)
  int bins[2 * PS];
  double w[2 * PS];
  const int spatialBins = 4, orientationBins = 8;
  int halfSize = PS >> 1;
  float step = float(spatialBins + 1) / (2 * halfSize);
  for (int i = 0; i < PS; i++) {
    float x = step * i;
    int xi = (int)(x);
    int b0 = xi - 1, b1 = xi;
    double w1 = x - xi;
    double w0 = 1.0f - w1;
    if (b0 < 0) { b0 = 0; w0 = 0; }
    if (b0 >= spatialBins) { b0 = spatialBins - 1; w0 = 0; }
    if (b1 < 0) { b1 = 0; w1 = 0; }
    if (b1 >= spatialBins) { b1 = spatialBins - 1; w1 = 0; }
    bins[i] = b0 * orientationBins; bins[PS + i] = b1 * orientationBins;
    w[i] = w0; w[PS + i] = w1;
    // k_describe forms (float)(w * (double)val) as an f32 product, which is the same number when w is an f32 value
    if ((double)(float)w0 != w0 || (double)(float)w1 != w1) { set_error("SIFT spatial weights are not f32 values"); return MODSX_ERR_ARG; }
  }
  MX_HIP(hipMalloc(&c->dSiftBins, sizeof bins));
  MX_HIP(hipMemcpy(c->dSiftBins, bins, sizeof bins, hipMemcpyHostToDevice));
  MX_HIP(hipMalloc(&c->dDescOrdered, 8));
  MX_HIP(hipMemset(c->dDescOrdered, 0, 8));
  { const char *e = getenv("MODSX_DESCRIBE_SLIM"); c->descSlim = !(e && atoi(e) == 0); }
  MX_HIP(hipMalloc(&c->dSiftW, sizeof w));
  MX_HIP(hipMemcpy(c->dSiftW, w, sizeof w, hipMemcpyHostToDevice));
  return MODSX_OK;
}

modsx_ctx *ctx_create(int device_id) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_error("no HIP device visible: libmodsx needs an MI355X (gfx950); there is no CPU fallback");
    return nullptr;
  }
  if (device_id < 0 || device_id >= ndev) { set_error("device id out of range"); return nullptr; }
  if (hipSetDevice(device_id) != hipSuccess) { set_error("hipSetDevice failed"); return nullptr; }
  {
    // How a host thread waits for its stream.  The runtime's default spins on the completion signal: with one context per host
    // thread that is one busy core per context for as long as the stream has work -- 16 contexts burn 16 cores, which is the
    // whole CPU allowance of a container limited to 16 CPUs (the hosts this library is benchmarked on: cpu.max 1600000 100000),
    // and the verification / component-tree threads then run into the cgroup's throttle (stalls of 60-90 ms per 100 ms period).
    // MODSX_SYNC=block (default) waits on the interrupt instead; MODSX_SYNC=spin keeps the runtime's default.
    // The flag is per DEVICE (and changes how every user of that device in this process waits): it is set once for each device a
    // context is made on.  A failure is reported once and is not fatal -- the runtime then keeps spinning.
    static std::once_flag once[64];
    if (device_id < 64)
      std::call_once(once[device_id], [device_id] {
        const char *e = getenv("MODSX_SYNC");
        if (e && !strcmp(e, "spin")) return;
        const unsigned flag = (e && !strcmp(e, "yield")) ? hipDeviceScheduleYield : hipDeviceScheduleBlockingSync;
        if (hipSetDeviceFlags(flag) != hipSuccess) {
          (void)hipGetLastError();
          fprintf(stderr, "modsx: hipSetDeviceFlags(hipDeviceScheduleBlockingSync) failed on device %d; host threads will spin-wait\n", device_id);
        }
      });
  }
  modsx_ctx *c = new modsx_ctx();
  c->dev = device_id;
  if (hipStreamCreate(&c->stream) != hipSuccess) { set_error("hipStreamCreate failed"); delete c; return nullptr; }
  for (int i = 0; i < 2; i++) hipEventCreateWithFlags(&c->descEv[i], hipEventDisableTiming);
  if (hipHostMalloc((void **)&c->hFlag, 64, hipHostMallocDefault) != hipSuccess) { set_error("hipHostMalloc failed"); hipStreamDestroy(c->stream); delete c; return nullptr; }
  c->hFlag[0] = 0; c->flagSeq = 0;
  c->waitRuntime = host_wait_runtime();
  for (int i = 0; i < 6; i++) c->timings[i] = 0;
  if (upload_tables(c) != MODSX_OK) { delete c; return nullptr; }
  return c;
}

void ctx_destroy(modsx_ctx *c) {
  if (!c) return;
  ctx_worker_stop(c);
  if (c->peer) { ctx_destroy(c->peer); c->peer = nullptr; }
  if (c->half) { ctx_destroy(c->half); c->half = nullptr; }
  hipSetDevice(c->dev);
  hipStreamSynchronize(c->stream);
  for (int i = 0; i < MAXB; i++) c->pyr[i].store.release();
  DevBuf *bufs[] = {&c->nmsJobs, &c->cand, &c->counter, &c->affJobs, &c->affOut, &c->oriJobs, &c->oriOut, &c->descJobs, &c->tilePrefix,
                    &c->taps, &c->imgRefs, &c->scratchA, &c->scratchB, &c->descAllF[0], &c->descAllF[1], &c->descAllU8[0],
                    &c->descAllU8[1], &c->descAllU8b[0], &c->descAllU8b[1], &c->shardLocal, &c->pos2, &c->matchRows, &c->matchWork, &c->dbSel, &c->misc, &c->scratchC, &c->needTab, &c->coordTab, &c->tileJob, &c->blurTiles, &c->nmsQueue, &c->rowStarts, &c->viewTmp[0], &c->viewTmp[1], &c->viewTaps, &c->viewJobs};
  for (DevBuf *b : bufs) b->release();
  for (int i = 0; i < MAXB; i++) { c->descF[i].release(); c->descU8[i].release(); c->viewImg[i].release(); for (int k = 0; k < 3; k++) c->descU8x[k][i].release(); }
  for (int d = 0; d < 2; d++) for (int t = 0; t < 4; t++) for (int sd = 0; sd < 2; sd++) c->descCls[d][t][sd].release();
  for (int t = 0; t < 4; t++) c->halfDesc[t].release();
  c->candSort.release(); c->candOut.release();
  c->patchBuf.release(); c->patchOut.release();
  c->liopTab.release(); c->liopDbg.release(); c->liopCnt.release();
  c->dspRows.release(); c->repStage.release();
  for (DevBuf &b : c->surfTab) b.release();
  for (DevBuf *b : {&c->sdInteg, &c->sdResp, &c->sdLap, &c->sdFlags, &c->sdCounts, &c->sdTab, &c->sdPoints, &c->sdExt}) b->release();
  c->sdHost.release(); c->sdBack.release();
  for (DevBuf *b : {&c->kzPlanes, &c->kzLdet, &c->kzTab, &c->kzHist, &c->kzFlags, &c->kzCounts, &c->kzRaw, &c->kzItems, &c->kzNine}) b->release();
  c->kzHost.release(); c->kzBack.release();
  for (DevBuf *b : {&c->claheTab, &c->clahePart, &c->claheLut, &c->claheDbg}) b->release();
  c->claheHost.release();
  for (DevBuf *b : {&c->caffeJobs, &c->caffeFlags, &c->caffeOut}) b->release();
  for (DevBuf &b : c->daisyTab) b.release();
  PinBuf *pins[] = {&c->hCand, &c->hAff, &c->hOri, &c->hDesc, &c->hMisc, &c->hNms, &c->hMatch, &c->hViewTaps, &c->hViewJobs, &c->hMser};
  for (PinBuf *b : pins) b->release();
  hipFree(c->dSmmMask); hipFree(c->dOriMask); hipFree(c->dOriIdx); hipFree(c->dSiftMask); hipFree(c->dSiftMaskIdx); hipFree(c->dAtan); hipFree(c->dOriBinTab); hipFree(c->dSiftOTab); hipFree(c->dSiftBins);
  hipFree(c->dSiftW); hipFree(c->dDescOrdered);
  for (int i = 0; i < 2; i++) hipEventDestroy(c->descEv[i]);
  c->hDescB.release(); c->hRefs.release();
  hipStreamDestroy(c->stream);
  if (c->hFlag) hipHostFree(c->hFlag);
  delete c;
}

static const double K_SIGMA = 2 * 3.0 * sqrt(3.0);  // synth-detection.cpp:28

// `Descriptors=` / `FGINNThreshold=` of the step: the step's own list, else the parameter block's, else {desc_type, match_ratio}
// ord[0..n): the classes of ds in descriptor-NAME order, the outer key of CorrespondencesMapMap (correspondencebank.cpp:117-179):
// "HalfRootSIFT" (3) < "HalfSIFT" (2) < "RootSIFT" (1) < "SIFT" (0)
void desc_class_order(const DescSet &ds, int *ord) {
  int m = 0;
  for (int type = 3; type >= 0; type--)
    for (int i = 0; i < ds.n; i++) if (ds.type[i] == type) ord[m++] = i;
}
int resolve_descs(const modsx_pair_params &pp, const modsx_ladder_step *st, DescSet &ds) {
  const int ns = st ? st->n_desc : 0;
  if (ns < 0 || ns > MODSX_MAX_DESC || pp.n_desc < 0 || pp.n_desc > MODSX_MAX_DESC) { set_error("n_desc must be 0..4"); return MODSX_ERR_ARG; }
  if (ns > 0) { ds.n = ns; for (int i = 0; i < ns; i++) { ds.type[i] = st->desc_types[i]; ds.ratio[i] = st->desc_ratios[i]; } }
  else if (pp.n_desc > 0) { ds.n = pp.n_desc; for (int i = 0; i < ds.n; i++) { ds.type[i] = pp.desc_types[i]; ds.ratio[i] = pp.desc_ratios[i]; } }
  else { ds.n = 1; ds.type[0] = pp.desc_type; ds.ratio[0] = st && st->match_ratio > 0 ? st->match_ratio : pp.match_ratio; }
  for (int i = 0; i < ds.n; i++) {
    if (ds.type[i] < 0 || ds.type[i] > 3) { set_error("descriptor type must be 0..3 (SIFT, RootSIFT, HalfSIFT, HalfRootSIFT)"); return MODSX_ERR_ARG; }
    for (int j = 0; j < i; j++) if (ds.type[j] == ds.type[i]) { set_error("a descriptor type is listed twice in one step"); return MODSX_ERR_ARG; }
  }
  return MODSX_OK;
}

static int upload_img_refs(modsx_ctx *c, const modsx_image *const *imgs, int n) {
  const bool fresh = !c->imgRefs.p;
  if (!c->imgRefs.ensure(MAXB * sizeof(ImgRef))) return MODSX_ERR_NOMEM;
  ImgRef refs[MAXB];
  memset(refs, 0, sizeof refs);
  for (int i = 0; i < n; i++) { refs[i].d = imgs[i]->d; refs[i].rows = imgs[i]->rows; refs[i].cols = imgs[i]->cols; }
  // orientation and description of a launch set name the same images: the table on the device is already right
  if (!fresh && memcmp(refs, c->imgRefsHost, sizeof refs) == 0) return MODSX_OK;
  // through a pinned copy of its own, in stream order and without a wait: the stream is idle when a stage begins (every stage ends
  // in a synchronize), so the previous table's copy has long completed when this buffer is written again
  if (!c->hRefs.ensure(sizeof refs)) return MODSX_ERR_NOMEM;
  memcpy(c->hRefs.p, refs, sizeof refs);
  MX_HIP(ctx_copy(c, c->imgRefs.p, c->hRefs.p, sizeof refs, hipMemcpyHostToDevice));
  memcpy(c->imgRefsHost, refs, sizeof refs);
  return MODSX_OK;
}

// ReprojectRegions' test for "H is the identity": the regions are copied, not transformed (synth-detection.cpp:549-560)
static double eye_test(const double *H) {
  return fabs(H[0] - 1.0) + fabs(H[1]) + fabs(H[2]) + fabs(H[3]) + fabs(H[4] - 1.0) + fabs(H[5]) + fabs(H[6]) + fabs(H[7]) +
         fabs(H[8] - 1.0);
}
static bool is_eye(const double *H) { return eye_test(H) < 0.01; }
// MODSX_ORI_PREFILTER=0: detect_orientation_batch launches every region that passes the view's border test (A/B runs, tests)
static bool ori_prefilter_on() {
  static const bool on = !(getenv("MODSX_ORI_PREFILTER") && atoi(getenv("MODSX_ORI_PREFILTER")) == 0);
  return on;
}
// measurement hook (modsx_debug_orientation_counts): orientation jobs launched, and regions left out because their reprojection
// is certain to drop them, by every context of the process since the last reset
static std::atomic<unsigned long long> g_oriLaunched{0}, g_oriSkipped{0};
// measurement hook (modsx_debug_orientation_launches): launches of the two instances of k_orientation, bin table in LDS / in
// global memory, by every context of the process since the last reset
static std::atomic<unsigned long long> g_oriLaunchLds{0}, g_oriLaunchGlobal{0};
void orientation_launches(unsigned long long *ldsTable, unsigned long long *globalTable, bool reset) {
  const unsigned long long a = reset ? g_oriLaunchLds.exchange(0) : g_oriLaunchLds.load();
  const unsigned long long b = reset ? g_oriLaunchGlobal.exchange(0) : g_oriLaunchGlobal.load();
  if (ldsTable) *ldsTable = a;
  if (globalTable) *globalTable = b;
}
void orientation_counts(unsigned long long *launched, unsigned long long *skipped, bool reset) {
  if (launched) *launched = reset ? g_oriLaunched.exchange(0) : g_oriLaunched.load();
  else if (reset) g_oriLaunched.store(0);
  if (skipped) *skipped = reset ? g_oriSkipped.exchange(0) : g_oriSkipped.load();
  else if (reset) g_oriSkipped.store(0);
}

// DetectOrientation, synth-detection.cpp:841-919, for a batch of (image, region list)
int detect_orientation_batch(modsx_ctx *c, const modsx_image *const *imgs, int n, const std::vector<modsx_region> *in,
                             double mrSize, int patchSize, int doHalfSIFT, int maxAngNum, double th, int addUpRight,
                             std::vector<modsx_region> *out, const OriReproj *reproj) {
  if (patchSize != 41) { set_error("orientation patchSize must be 41"); return MODSX_ERR_ARG; }
  const bool prefilter = reproj && ori_prefilter_on();
  for (int i = 0; i < n; i++) out[i].clear();
  double mrScale = (double)mrSize;
  int patchImageSize = 2 * int(mrScale) + 1;
  double imageToPatchScale = double(patchImageSize) / (double)patchSize;
  HostMark hm;
  std::vector<OriJob> jobs;
  std::vector<char> passed[MAXB];
  std::vector<unsigned char> certain[MAXB];   // reproj: the caller's reproject_regions drops the region whatever its angle turns out to be
  std::vector<OriJob> jobsOf[MAXB];     // per image, then concatenated: the images are independent (one pool task each)
  host_parallel_light(n, [&](int i) {
    passed[i].assign(in[i].size(), 0);
    jobsOf[i].clear();
    jobsOf[i].reserve(in[i].size());
    // (the identity onto the view's own size repeats the test below on the rotated shape: a region that passes it unrotated has
    // |a11| + |a12| >= the row norm inside the bounds and is never certain to be dropped -- nothing to compute)
    const bool sameTest = prefilter && reproj[i].orig_w == imgs[i]->cols && reproj[i].orig_h == imgs[i]->rows && is_eye(reproj[i].H);
    if (prefilter && !sameTest) {
      certain[i].resize(in[i].size());
      reproject_certain_drop(in[i].data(), (int)in[i].size(), reproj[i].H, reproj[i].orig_w, reproj[i].orig_h, K_SIGMA, certain[i].data());
    }
    unsigned long long nSkipped = 0;
    for (size_t r = 0; r < in[i].size(); r++) {
      const modsx_keypoint &k = in[i][r].det_kp;
      if (check_borders_host(imgs[i]->cols, imgs[i]->rows, (float)k.x, (float)k.y, (float)k.a11, (float)k.a12,
                             (float)k.a21, (float)k.a22, (int)(K_SIGMA * k.s), (int)(K_SIGMA * k.s)))
        continue;
      if (!certain[i].empty() && certain[i][r]) { nSkipped++; continue; }   // like a region at the view's border: no job, no output
      passed[i][r] = 1;
      if (maxAngNum > 0) {
        float curr_sc = imageToPatchScale * k.s;
        OriJob j;
        j.img = i; j.x = (float)k.x; j.y = (float)k.y;
        j.a11 = (float)k.a11 * curr_sc; j.a12 = (float)k.a12 * curr_sc;
        j.a21 = (float)k.a21 * curr_sc; j.a22 = (float)k.a22 * curr_sc;
        jobsOf[i].push_back(j);
      }
    }
    if (nSkipped) g_oriSkipped.fetch_add(nSkipped, std::memory_order_relaxed);
  });
  size_t jobStart[MAXB + 1];
  jobStart[0] = 0;
  for (int i = 0; i < n; i++) jobStart[i + 1] = jobStart[i] + jobsOf[i].size();
  jobs.resize(jobStart[n]);
  g_oriLaunched.fetch_add(jobStart[n], std::memory_order_relaxed);
  host_parallel_light(n, [&](int i) { if (!jobsOf[i].empty()) memcpy(jobs.data() + jobStart[i], jobsOf[i].data(), jobsOf[i].size() * sizeof(OriJob)); });
  hm.mark("orientation jobs");
  const float *res = nullptr;   // in the pinned staging buffer: (1 + maxA) words per job
  const int maxA = maxAngNum < 0 ? ORI_MAX_PEAKS : std::min(maxAngNum, ORI_MAX_PEAKS);
  const size_t oriB = (size_t)(1 + maxA) * 4;
  if (!jobs.empty()) {
    int rc = upload_img_refs(c, imgs, n);
    if (rc) return rc;
    hipStream_t s = c->stream;
    size_t nj = jobs.size();
    if (!c->oriJobs.ensure(nj * sizeof(OriJob)) || !c->oriOut.ensure(nj * oriB) ||
        !c->hOri.ensure(nj * (sizeof(OriJob) + oriB)))
      return MODSX_ERR_NOMEM;
    // jobs up and results down through pinned memory: pageable transfers are staged and serialised by the runtime
    memcpy(c->hOri.p, jobs.data(), nj * sizeof(OriJob));
    float *hres = (float *)((char *)c->hOri.p + nj * sizeof(OriJob));
    res = hres;
    MX_HIP(ctx_copy(c, c->oriJobs.p, c->hOri.p, nj * sizeof(OriJob), hipMemcpyHostToDevice));
    ProfScope ps(c, K_ORIENT, (double)nj * 41 * 41 * 4);
    (orientation_lds_table((int)nj) ? g_oriLaunchLds : g_oriLaunchGlobal).fetch_add(1, std::memory_order_relaxed);
    launch_orientation(s, (OriJob *)c->oriJobs.p, (float *)c->oriOut.p, (int)nj, (ImgRef *)c->imgRefs.p, c->dOriIdx,
                       c->dOriMask, c->dOriBinTab, doHalfSIFT, th, maxA);
    MX_HIP(ctx_copy(c, hres, c->oriOut.p, nj * oriB, hipMemcpyDeviceToHost));
    MX_HIP(ctx_sync(c));
  }
  hm.mark("orientation launch + wait");
  host_parallel_light(n, [&](int i) {
    size_t jk = jobStart[i];
    out[i].clear();
    out[i].reserve(in[i].size() + in[i].size() / 4);
    for (size_t r = 0; r < in[i].size(); r++) {
      if (!passed[i][r]) continue;
      // (a region is a 200-byte record: it is copied once, into its place in the list, and edited there)
      const modsx_region &base = in[i][r];
      if (maxAngNum > 0) {
        const float *o = res + (jk++) * (size_t)(1 + maxA);
        int on;
        memcpy(&on, o, 4);
        const double b11 = base.det_kp.a11, b12 = base.det_kp.a12, b21 = base.det_kp.a21, b22 = base.det_kp.a22;
        for (int a = 0; a < on; a++) {
          // `using namespace std` in synth-detection.cpp:30 => cos/sin(float) are the f32 overloads
          double ci = cosf(-o[1 + a]);
          double si = sinf(-o[1 + a]);
          out[i].push_back(base);
          modsx_region &t = out[i].back();
          t.id = 0;  // const_temp_region.id = count, count is never incremented (synth-detection.cpp:854,889)
          t.det_kp.a11 = b11 * ci - b12 * si;
          t.det_kp.a12 = b11 * si + b12 * ci;
          t.det_kp.a21 = b21 * ci - b22 * si;
          t.det_kp.a22 = b21 * si + b22 * ci;
        }
      }
      if (addUpRight) { out[i].push_back(base); if (maxAngNum > 0) out[i].back().id = 0; }
    }
  });
  hm.mark("rotated regions");
  return MODSX_OK;
}

// ReprojectRegions, synth-detection.cpp:541-616 (box = k_sigma * s), and ReprojectRegionsAndRemoveTouchBoundary, :63-102
// (box = mrSize * s, default 3 sqrt 3: the "None" list of imagerepresentation.cpp:1271-1272)
int reproject_regions(modsx_region *regs, int n, const double *H, int orig_w, int orig_h) {
  return reproject_regions_box(regs, n, H, orig_w, orig_h, K_SIGMA);
}
int reproject_regions_box(modsx_region *regs, int n, const double *H, int orig_w, int orig_h, double boxk) {
  double eyeTest = eye_test(H);
  double Hi[9];
  invert3(H, Hi);
  for (int i = 0; i < n; i++) {
    regs[i].reproj_kp = regs[i].det_kp;
    if (!(eyeTest < 0.01)) {
      const modsx_keypoint k = regs[i].det_kp;
      modsx_keypoint &o = regs[i].reproj_kp;
      o.x = (Hi[0] * k.x + Hi[1] * k.y + Hi[2]);
      o.y = (Hi[3] * k.x + Hi[4] * k.y + Hi[5]);
      o.a11 = (Hi[0] * k.a11 + Hi[1] * k.a21);
      o.a12 = (Hi[0] * k.a12 + Hi[1] * k.a22);
      o.a21 = (Hi[3] * k.a11 + Hi[4] * k.a21);
      o.a22 = (Hi[3] * k.a12 + Hi[4] * k.a22);
    }
  }
  int m = 0;
  for (int i = 0; i < n; i++) {
    const modsx_keypoint &k = regs[i].reproj_kp;
    if ((k.x < orig_w) && (k.y < orig_h) && (k.x > 0) && (k.y > 0)) {
      if (!check_borders_host(orig_w, orig_h, (float)k.x, (float)k.y, (float)k.a11, (float)k.a12, (float)k.a21,
                              (float)k.a22, (int)(boxk * k.s), (int)(boxk * k.s)))
      { if (m != i) regs[m] = regs[i]; m++; }
    }
  }
  return m;
}

// drop[i] = 1 when reproject_regions_box(..., H, orig_w, orig_h, boxk) removes region i after ANY rotation of its shape matrix
// from the right (what detect_orientation_batch does with the dominant angles), 0 when that is not certain.
//
// The centre test does not read the shape: it is evaluated here by the exact path's own expressions.  For the box, with
// M = Hinv_lin * A and a rotation R, the corners lie at x' +- hw * m11' +- hw * m12' with (m11', m12') = row 1 of M * R, and
// |m11'| + |m12'| >= ||row 1 of M * R|| = ||row 1 of M||: the largest corner offset in x is at least dx = |hw| * ||row 1 of M||
// whatever the angle, the same in y with row 2.  The region is certainly dropped when x' + dx > w - 3, x' - dx < 1,
// y' + dy > h - 3 or y' - dy < 1 hold with a margin for the rounding of the exact path (u = 2^-24, T = |x'| + sqrt 2 * dx
// bounds |x'| + |hw| * (|m11'| + |m12'|)):
//  * cosf / sinf are within 1 ulp, taken as 2^-23 per entry: the applied matrix is R + E with ||E||_2 <= 2^-22, the row norm
//    shrinks by at most dx * 4u;
//  * the f64 products of the rotation and of Hinv_lin * (A * R), four roundings on sums of two products each: at most
//    e64 = |hw| * 2^-50 * (|Hi_r0| + |Hi_r1|) * (|a11| + |a12| + |a21| + |a22|) in a corner coordinate (no cancellation assumed);
//  * the casts of x', m11', m12' to f32, the two f32 products and the two f32 additions of check_borders: every term of the
//    corner carries at most four factors (1 + u), at most 4u * T.
// Together less than B = 4u * (|x'| + 3 * dx) + e64.  The margin is 32 * B (2^-17 * (|x'| + 3 * dx) + 32 * e64, 0.01 px for a
// 1024 px image): too generous a margin only narrows the caught band by that much.  Anything not finite, a box size beyond
// int and magnitudes near the end of the f32 range are "not certain".
void reproject_certain_drop(const modsx_region *regs, int n, const double *H, int orig_w, int orig_h, double boxk, unsigned char *drop) {
  const bool eye = is_eye(H);
  double Hi[9];
  invert3(H, Hi);
  const double lim[2] = {(double)(float)(orig_w - 3), (double)(float)(orig_h - 3)};   // check_borders: width - 1, height - 1
  for (int i = 0; i < n; i++) {
    drop[i] = 0;
    const modsx_keypoint &k = regs[i].det_kp;
    double c[2] = {k.x, k.y};
    double m[2][2] = {{k.a11, k.a12}, {k.a21, k.a22}};
    double hi1[2] = {1.0, 1.0};    // |Hi_r0| + |Hi_r1| of the row (the identity view copies the shape: no products, e64 over-estimates)
    if (!eye) {
      c[0] = (Hi[0] * k.x + Hi[1] * k.y + Hi[2]);
      c[1] = (Hi[3] * k.x + Hi[4] * k.y + Hi[5]);
      m[0][0] = (Hi[0] * k.a11 + Hi[1] * k.a21);
      m[0][1] = (Hi[0] * k.a12 + Hi[1] * k.a22);
      m[1][0] = (Hi[3] * k.a11 + Hi[4] * k.a21);
      m[1][1] = (Hi[3] * k.a12 + Hi[4] * k.a22);
      hi1[0] = fabs(Hi[0]) + fabs(Hi[1]);
      hi1[1] = fabs(Hi[3]) + fabs(Hi[4]);
    }
    const double box = boxk * k.s;
    const double a1 = fabs(k.a11) + fabs(k.a12) + fabs(k.a21) + fabs(k.a22);
    if (!std::isfinite(c[0]) || !std::isfinite(c[1]) || !std::isfinite(m[0][0] + m[0][1] + m[1][0] + m[1][1]) || !std::isfinite(a1) ||
        !std::isfinite(hi1[0] + hi1[1]) || !(fabs(box) < 2e9))
      continue;
    // far inside the f32 range, or check_borders may meet inf - inf: a NaN corner compares false and keeps the region
    if (!(fabs(c[0]) + fabs(c[1]) + fabs(m[0][0]) + fabs(m[0][1]) + fabs(m[1][0]) + fabs(m[1][1]) < 1e25)) continue;
    if (!((c[0] < orig_w) && (c[1] < orig_h) && (c[0] > 0) && (c[1] > 0))) { drop[i] = 1; continue; }
    const double hw = fabs((double)(float)ceil((double)(float)(int)box / 2.0));    // check_borders' hw of res_w = (int)(boxk * s)
    for (int r = 0; r < 2; r++) {
      const double d = hw * sqrt(m[r][0] * m[r][0] + m[r][1] * m[r][1]);
      const double e64 = hw * 0x1p-50 * hi1[r] * a1;
      const double margin = 0x1p-17 * (fabs(c[r]) + 3.0 * d) + 32.0 * e64;
      if (!std::isfinite(d) || !std::isfinite(margin)) continue;
      if (c[r] - d < 1.0 - margin || c[r] + d > lim[r] + margin) drop[i] = 1;
    }
  }
}

// One planned chunk of describe_batch on the device: its blob staged through pinned slot `slot` (two in turn: the copy of chunk k
// may still be in flight while chunk k + 1 is being prepared), then the launch set.
static int launch_describe_chunk(modsx_ctx *c, const DescChunkPlan &cp, int slot, HostMark &hm, int photoNorm, const DescSet &ds,
                                 double maxBin, const DescOut &outs, const DescTail *tail) {
  hipStream_t s = c->stream;
  const size_t nj = cp.jobs.size();
  const int nS = cp.pfxSample.back(), nR = cp.pfxRow.back(), nC = cp.pfxCol.back(), nRL = cp.pfxRowL.back(), nCL = cp.pfxColL.back();
  const DescBlobLayout L(cp);
  PinBuf &hblob = slot ? c->hDescB : c->hDesc;
  if (c->descEvPending[slot]) { MX_HIP(c->descByEvent[slot] ? hipEventSynchronize(c->descEv[slot]) : ctx_wait_mark(c, c->descMark[slot])); c->descEvPending[slot] = false; }
  if (!c->descJobs.ensure(L.devB) || !hblob.ensure(L.blobB) ||
      !c->scratchA.ensure(std::max<size_t>(1, cp.arenaA) * 4) || !c->scratchB.ensure(std::max<size_t>(1, cp.arenaB) * 4) ||
      !c->scratchC.ensure(std::max<size_t>(1, cp.arenaC) * 4) || !c->rowStarts.ensure(std::max<size_t>(1, cp.rowStarts) * 8) ||
      !c->tileJob.ensure(((size_t)nS + nR + nC + 3) * 4))
    return MODSX_ERR_NOMEM;
  int *tjS = (int *)c->tileJob.p, *tjR = tjS + nS, *tjC = tjR + nR;
  if (!c->blurTiles.ensure(((size_t)nRL + nCL + 1) * sizeof(BlurTile))) return MODSX_ERR_NOMEM;
  BlurTile *btR = (BlurTile *)c->blurTiles.p, *btC = btR + nRL;
  char *hb = (char *)hblob.p, *db = (char *)c->descJobs.p;
  describe_fill_blob(cp, L, hb);
  hm.mark("desc tables + blob");
  MX_HIP(ctx_copy(c, db, hb, L.blobB, hipMemcpyHostToDevice));
  c->descByEvent[slot] = c->waitRuntime || !c->hFlag;
  if (c->descByEvent[slot]) MX_HIP(hipEventRecord(c->descEv[slot], s)); else c->descMark[slot] = ctx_mark(c);
  c->descEvPending[slot] = true;
  int *dPfxS = (int *)(db + L.pfx(0)), *dPfxR = (int *)(db + L.pfx(1)), *dPfxC = (int *)(db + L.pfx(2));
  int *dPfxRL = (int *)(db + L.pfx(3)), *dPfxCL = (int *)(db + L.pfx(4));
  float *dTaps = (float *)(db + L.oTaps), *dCoord = (float *)(db + L.oCoord);
  int *dNeed = (int *)(db + L.oNeed);
  const DescJob *dj = (const DescJob *)(db + L.oJobs);
  // tile -> job tables of the global-memory fallbacks: most chunks have no such tiles at all
  if (nS) launch_expand_tiles(s, dPfxS, (int)nj, tjS);
  if (nR) launch_expand_tiles(s, dPfxR, (int)nj, tjR);
  if (nC) launch_expand_tiles(s, dPfxC, (int)nj, tjC);
  // algorithmic work of the describe STAGE per SURVEY section 8(d): the (P+2)^2 f32 window of every region read once
  // (booked here) + 128 B written per region (booked on k_describe); the arenas between the four kernels are an
  // artefact of the split and are not algorithmic bytes
  if (nRL + nCL)
    launch_expand_blur_tiles(s, dj, dPfxRL, dPfxCL, (int)nj, dNeed, btR, btC, (float2 *)c->rowStarts.p);
  { ProfScope ps(c, K_PATCH_SAMPLE, (double)cp.windowFloats * 4);
    launch_sample_rows(s, dj, btR, nRL, (ImgRef *)c->imgRefs.p, dTaps, dNeed, (float *)c->scratchB.p,
                       (const float2 *)c->rowStarts.p, (float *)c->scratchC.p);
    launch_patch_sample(s, dj, dPfxS, tjS, nS, (ImgRef *)c->imgRefs.p, (float *)c->scratchA.p); }
  { ProfScope ps(c, K_BLUR_ROWS, 0.0);
    launch_patch_blur(s, dj, dPfxR, tjR, nR, dTaps, dNeed, (float *)c->scratchA.p,
                      (float *)c->scratchB.p, 0); }
  { ProfScope ps(c, K_BLUR_COLS, 0.0);
    launch_blur_cols(s, btC, nCL, dTaps, dNeed, (float *)c->scratchB.p, (float *)c->scratchC.p);
    launch_patch_blur(s, dj, dPfxC, tjC, nC, dTaps, dNeed, (float *)c->scratchB.p,
                      (float *)c->scratchC.p, 1); }
  // the patch-out callers (engine_liop.hip): the normalised patches of the chunk's jobs instead of their SIFT descriptors
  if (tail) return tail->run(c, tail->self, dj, (int)nj, (const float *)c->scratchC.p, dNeed, dCoord, photoNorm);
  ProfScope psd(c, K_DESCRIBE, (double)nj * 128 * ds.n);
  // a chunk without a direct-branch job: the slim form, its redo list behind the blob (MODSX_DESCRIBE_SLIM=0: never)
  unsigned *const redo = cp.slim && c->descSlim ? (unsigned *)(db + L.oRedo) : nullptr;
  const int slim = launch_describe(s, dj, (int)nj, (ImgRef *)c->imgRefs.p, (float *)c->scratchC.p, dNeed, dCoord,
                                   c->dSiftMask, c->dSiftMaskIdx, c->nSiftMask, c->dSiftOTab,
                                   c->dSiftBins, c->dSiftW, photoNorm, ds.packed(), ds.n, maxBin, outs, c->dDescOrdered, redo);
  c->descSlimCnt[slim ? 0 : 1]++;
  return MODSX_OK;
}

// DescribeRegions<SIFTDescriptor>, synth-detection.hpp:169-255, for a batch.  Descriptors stay in HBM
// (c->descF[i], c->descU8[i]); descHost[i] (optional) receives the f32 copy.
static int describe_batch_impl(modsx_ctx *c, const modsx_image *const *imgs, int n, const std::vector<modsx_region> *regs,
                               double mrSize, int patchSize, int fast, int photoNorm, int descType, double maxBin,
                               float *const *descHost, float *const *devF, uint8_t *const *devU8, const DescSet *ds,
                               uint8_t *const *const *devU8x, const DescTail *tail) {
  if (patchSize != 41) { set_error("descriptor patchSize must be 41"); return MODSX_ERR_ARG; }
  DescSet one;
  if (!ds) { one.n = 1; one.type[0] = descType; ds = &one; }
  if (ds->n < 1 || ds->n > MODSX_MAX_DESC) { set_error("describe: 1..4 descriptor classes"); return MODSX_ERR_ARG; }
  if (n > MAXB) { set_error("describe batch too large"); return MODSX_ERR_ARG; }
  hipStream_t s = c->stream;
  int rc = upload_img_refs(c, imgs, n);
  if (rc) return rc;
  // Window arena per chunk.  Measured on MI355X with 16 contexts: throughput is flat up to 256 MiB per context and
  // halves from 384 MiB on (the three arenas of all contexts stop fitting the 256 MiB Infinity Cache working set),
  // so a batch is cut into chunks of 192 MiB of windows.  MODSX_ARENA_MB overrides it for experiments.
  static const size_t arenaMB = getenv("MODSX_ARENA_MB") ? (size_t)atol(getenv("MODSX_ARENA_MB")) : 192;
  const size_t ARENA_FLOATS = std::max<size_t>(arenaMB, 16) << 18;  // MiB -> floats
  DescOut outs;
  memset(&outs, 0, sizeof outs);
  for (int i = 0; i < n && !tail; i++) {
    const size_t nr = regs[i].size();
    float *outF = devF ? devF[i] : nullptr;
    uint8_t *outU8 = devU8 ? devU8[i] : nullptr;
    if (!outF) { if (!c->descF[i].ensure(std::max<size_t>(1, nr) * 128 * 4)) return MODSX_ERR_NOMEM; outF = (float *)c->descF[i].p; }
    if (!outU8) { if (!c->descU8[i].ensure(std::max<size_t>(1, nr) * 128)) return MODSX_ERR_NOMEM; outU8 = (uint8_t *)c->descU8[i].p; }
    outs.f[i] = outF; outs.u8[i] = outU8;
    for (int k = 1; k < ds->n; k++) {
      uint8_t *o = devU8x && devU8x[k - 1] ? devU8x[k - 1][i] : nullptr;
      if (!o) { if (!c->descU8x[k - 1][i].ensure(std::max<size_t>(1, nr) * 128)) return MODSX_ERR_NOMEM; o = (uint8_t *)c->descU8x[k - 1][i].p; }
      outs.u8x[k - 1][i] = o;
    }
  }
  // the regions of all images of the batch go through one launch set per chunk (a chunk ends when the window arena is
  // full); region order inside an image is kept, outIdx addresses the image's own descriptor buffer.  What a chunk holds is
  // planned on the host (describe_plan.cpp), one chunk at a time: chunk k + 1 is planned and staged while chunk k runs
  HostMark hm;
  DescBatch batch;
  batch.regs = regs; batch.n = n; batch.mrSize = mrSize; batch.fast = fast;
  DescCursor cur = describe_windows(batch);
  int chunkNo = 0;
  c->descCnt[DC_CALLS]++;
  for (; cur.img < n; chunkNo++) {
    DescChunkPlan cp;
    const int prc = describe_plan_chunk(batch, cur, ARENA_FLOATS, cp, hm);
    for (int q = 0; q < DC_N; q++) c->descCnt[q] += cp.cnt[q];
    if (prc) return prc;
    rc = launch_describe_chunk(c, cp, chunkNo & 1, hm, photoNorm, *ds, maxBin, outs, tail);
    if (rc) return rc;
    cur = cp.next;
  }
  c->descCnt[DC_MAX_CHUNKS] = std::max<long>(c->descCnt[DC_MAX_CHUNKS], chunkNo);
  hm.mark("desc launches");
  MX_HIP(ctx_sync(c));   // callers read the descriptor buffers and reuse the staging blobs
  hm.mark("desc wait");
  c->descEvPending[0] = c->descEvPending[1] = false;
  if (descHost && !tail) {
    bool any = false;
    for (int i = 0; i < n; i++)
      if (descHost[i] && !regs[i].empty()) {
        MX_HIP(hipMemcpyAsync(descHost[i], outs.f[i], regs[i].size() * 128 * 4, hipMemcpyDeviceToHost, s));
        any = true;
      }
    if (any) MX_HIP(hipStreamSynchronize(s));
  }
  MX_HIP(hipGetLastError());
  return MODSX_OK;
}

int describe_batch(modsx_ctx *c, const modsx_image *const *imgs, int n, const std::vector<modsx_region> *regs,
                   double mrSize, int patchSize, int fast, int photoNorm, int descType, double maxBin,
                   float *const *descHost, float *const *devF, uint8_t *const *devU8, const DescSet *ds,
                   uint8_t *const *const *devU8x) {
  return describe_batch_impl(c, imgs, n, regs, mrSize, patchSize, fast, photoNorm, descType, maxBin, descHost, devF, devU8, ds, devU8x,
                             nullptr);
}
// one image's regions through the same windows, planner and launch sets, with `tail` in place of k_describe; returns after the
// stream has drained
int describe_batch_tail(modsx_ctx *c, const modsx_image *img, const std::vector<modsx_region> &regs, double mrSize, int patchSize,
                        int fast, int photoNorm, const DescTail &tail) {
  const modsx_image *imgs[1] = {img};
  return describe_batch_impl(c, imgs, 1, &regs, mrSize, patchSize, fast, photoNorm, MODSX_DESC_ROOT_SIFT, 0.2, nullptr, nullptr, nullptr,
                             nullptr, nullptr, &tail);
}

// the host half of the matcher: per-query result rows -> TentativeCorrespExt records (matching.cpp:435-457)
// ddb (optional): the squared distance of every query to its nearest database descriptor (BIG where no record can arise) turns
// the records into MatchFlannFGINNPlusDB's (matching.cpp:462-572).  ratioDB = d0 / dDB does not depend on j, so the database
// variant yields the plain records filtered and relabelled: with `max` = std::max, max(r_j, rDB) is rDB iff r_j < rDB (a NaN
// rDB -- the query sits ON its nearest train and ON a database row -- leaves r_j), and a record survives iff that maximum
// is <= ratio^2.  In the "all points" branch (ratio >= 1, :505-536) the records are the plain ones plus d2byDB.
void rows_to_tentatives(const MatchRow *rows, int n1, int nn, std::vector<modsx_tentative> &o, const int *ddb, double sqminratio,
                        std::vector<double> *d2byDB) {
  o.reserve(n1 / 4 + 16);
  if (d2byDB) d2byDB->clear();
  for (int q = 0; q < n1; q++) {
    const MatchRow &r = rows[q];
    // rank of the first ratio-passing neighbour is nless+1; it must be <= nn-1 and every neighbour
    // before it must lie within contradDist of NN0 (matching.cpp:435-457)
    if (r.t0 < 0 || r.tj < 0 || r.nbad != 0 || r.nless > nn - 2) continue;
    modsx_tentative t;
    t.q = q; t.t0 = r.t0; t.tj = r.tj;
    t.t1 = r.t1;
    t.d1 = r.d0; t.d2 = r.dj; t.d2by2ndcl = r.d1;
    double ratio = r.d0 / r.dj;  // f32 / f32, then widened (matching.cpp:437)
    if (ddb) {
      const float dDB = (float)ddb[q];                 // an integer below 2^24: exact
      if (sqminratio < 1.0) {
        const double ratioDB = r.d0 / dDB;             // f32 / f32, then widened (:544)
        if (ratio < ratioDB) ratio = ratioDB;          // std::max(ratio, ratioDB) (:548)
        if (!(ratio <= sqminratio)) continue;          // (:549)
      }
      if (d2byDB) d2byDB->push_back((double)dDB);
    }
    t.ratio = sqrt(ratio);
    o.push_back(t);
  }
}

// MatchFlannFGINN (matching/matching.cpp:357-461, linear index) on descriptors resident in HBM, for nb <= MATCH_MAXB
// independent (query set, train set) problems that share the kernel launches (blockIdx.z) and one synchronisation
int match_device_batch(modsx_ctx *c, int nb, const uint8_t *const *d1, const int *n1, const uint8_t *const *d2, const int *n2,
                       const double *const *pos2Host, double ratioT, double contradDist, int nn,
                       std::vector<modsx_tentative> *out, const MatchShard *shard, const double *const *pos2Dev, const DbSet *db,
                       std::vector<double> *d2byDB, const void *const *trainPack) {
  // pos2Dev (optional, unsharded branch): the positions already live on the device; pos2Host is then not read
  // trainPack (optional, unsharded branch): trainPack[i] != nullptr = the trains of problem i were packed there, with their
  // positions (a stored image representation): d2[i] and the positions of that problem are not read, nothing is uploaded for it
  // db (optional, unsharded branch): MatchFlannFGINNPlusDB -- behind the matcher's launches, on the same stream, the queries that
  // give a record are selected and swept against the database (kernels_dbnn.hip); their dDB words travel down with the rows
  CtxBusy busy(c);
  if (nb < 1 || nb > MATCH_MAXB) { set_error("match_device_batch: batch size"); return MODSX_ERR_ARG; }
  hipStream_t s = c->stream;
  const double sqminratio = ratioT * ratioT, contrDistSq = contradDist * contradDist;
  if (!(sqminratio == sqminratio)) { set_error("match ratio is NaN"); return MODSX_ERR_ARG; }   // ratio >= 1: the "all points" branch (matching.cpp:397-428)
  // nn = neighbours the walk may look at (default 50, matching.hpp:268-269); the event lists of the device matcher hold up to MATCH_NN_MAX groups
  if (nn < 2 || nn > MATCH_NN_MAX) { set_error("match: nn must be in [2, 256]"); return MODSX_ERR_ARG; }
  for (int i = 0; i < nb; i++)      // the matcher logs train tiles as 16-bit numbers (kernels_match.hip k_match_resolve)
    if (n2[i] > 2000000) { set_error("match: more than 2 000 000 train descriptors in one problem"); return MODSX_ERR_ARG; }
  if (shard) {
    // view-sharded run (engine_shard.hip): this rank matches the query rows [lo, lo + per) of ONE problem; the result rows
    // of all ranks are all-gathered on the device and every rank builds the full tentative list
    if (nb != 1) { set_error("match_device_batch: a sharded match takes one problem"); return MODSX_ERR_ARG; }
    if (db) { set_error("match_device_batch: a sharded match takes no descriptor database"); return MODSX_ERR_ARG; }
    out[0].clear();
    const int N1 = shard->n1_total, M = n2[0], per = shard->per;
    const int lo = shard->lo, nloc = std::max(0, std::min(N1, lo + per) - lo);
    MatchRow *blk = nullptr;
    int rc = match_shard_begin(c, *shard, &blk);          // the lane's blocks (growth agreed by all ranks)
    if (rc) return rc;
    // from here to the all-gather nothing returns: a local failure travels in the block header
    int lrc = MODSX_OK;
    const int world = shard->world;
    const size_t posB = align_up((size_t)M * 16, 256), allB = (size_t)world * (per + 1) * sizeof(MatchRow);
    if (!c->pos2.ensure(posB) || !c->hMatch.ensure(posB + align_up(allB, 256)) || !c->matchWork.ensure(match_workspace_bytes(std::max(1, nloc), M)))
      lrc = MODSX_ERR_NOMEM;
    char *hpos = (char *)c->hMatch.p, *hrow = hpos ? hpos + posB : nullptr;
    if (!lrc) {
      memcpy(hpos, pos2Host[0], (size_t)M * 16);
      if (ctx_copy(c, c->pos2.p, hpos, (size_t)M * 16, hipMemcpyHostToDevice) != hipSuccess) { set_error("sharded match: upload failed"); lrc = MODSX_ERR_DEVICE; }
    }
    if (!lrc && nloc > 0) {
      ProfScope ps(c, K_MATCH, 2.0 * nloc * (double)M * 128);
      launch_match(s, d1[0] + (size_t)lo * 128, nloc, d2[0], M, (const double *)c->pos2.p, sqminratio, contrDistSq, nn, blk + 1, c->matchWork.p);
    }
    rc = match_shard_gather(c, *shard, lrc, lrc ? nullptr : (MatchRow *)hrow);
    if (rc) return rc;
    // rank r's rows sit behind its header row; the last ranks may hold fewer rows, or none
    std::vector<MatchRow> rows((size_t)N1);
    for (int r = 0; r < world; r++) {
      const int rlo = std::min(N1, r * per), rn = std::min(N1, rlo + per) - rlo;
      if (rn > 0) memcpy(rows.data() + rlo, (const MatchRow *)hrow + (size_t)r * (per + 1) + 1, (size_t)rn * sizeof(MatchRow));
    }
    rows_to_tentatives(rows.data(), N1, nn, out[0]);
    return MODSX_OK;
  }
  if (db && db->dev != c->dev) { set_error("match: the descriptor database lives on another device"); return MODSX_ERR_ARG; }
  size_t posOfs[MATCH_MAXB], rowOfs[MATCH_MAXB], workOfs[MATCH_MAXB], posB = 0, rowB = 0, workB = 0;
  int live[MATCH_MAXB], nl = 0;
  for (int i = 0; i < nb; i++) {
    out[i].clear();
    if (d2byDB) d2byDB[i].clear();
    if (n1[i] <= 0 || n2[i] <= 0) continue;
    posOfs[nl] = posB;
    if (!(trainPack && trainPack[i])) posB += align_up((size_t)n2[i] * 16, 256);
    rowOfs[nl] = rowB; rowB += align_up((size_t)n1[i] * sizeof(MatchRow), 256);
    workOfs[nl] = workB; workB += align_up(match_workspace_bytes(n1[i], n2[i]), 256);
    live[nl++] = i;
  }
  if (!nl) return MODSX_OK;
  // with a database: dDB per query behind the rows (one download), the selected-query lists and their counts in a buffer of their own
  size_t ddbOfs[MATCH_MAXB], selOfs[MATCH_MAXB], selB = 256;
  if (db)
    for (int k = 0; k < nl; k++) {
      ddbOfs[k] = rowB; rowB += align_up((size_t)n1[live[k]] * 4, 256);
      selOfs[k] = selB; selB += align_up((size_t)n1[live[k]] * 4, 256);
    }
  if (!c->pos2.ensure(posB) || !c->matchRows.ensure(rowB) || !c->matchWork.ensure(workB) || !c->hMatch.ensure(posB + rowB) ||
      (db && !c->dbSel.ensure(selB)))
    return MODSX_ERR_NOMEM;
  char *hpos = (char *)c->hMatch.p, *hrow = hpos + posB;   // pinned staging: positions up, rows down
  const uint8_t *pd1[MATCH_MAXB], *pd2[MATCH_MAXB];
  const double *ppos[MATCH_MAXB];
  MatchRow *prow[MATCH_MAXB];
  void *pwork[MATCH_MAXB];
  const void *ppack[MATCH_MAXB];
  int pn1[MATCH_MAXB], pn2[MATCH_MAXB];
  double work = 0;
  for (int k = 0; k < nl; k++) {
    const int i = live[k];
    pd1[k] = d1[i]; pd2[k] = d2[i]; pn1[k] = n1[i]; pn2[k] = n2[i];
    ppack[k] = trainPack ? trainPack[i] : nullptr;
    ppos[k] = ppack[k] ? nullptr : pos2Dev ? pos2Dev[i] : (const double *)((char *)c->pos2.p + posOfs[k]);
    prow[k] = (MatchRow *)((char *)c->matchRows.p + rowOfs[k]);
    pwork[k] = (char *)c->matchWork.p + workOfs[k];
    if (!pos2Dev && !ppack[k]) memcpy(hpos + posOfs[k], pos2Host[i], (size_t)n2[i] * 16);
    work += 2.0 * n1[i] * (double)n2[i] * 128;
  }
  if (!pos2Dev && posB) MX_HIP(ctx_copy(c, c->pos2.p, hpos, posB, hipMemcpyHostToDevice));
  {
    // K_MATCH = every launch of the problem(s); K_MATCH_SWEEP1 = the one launch that carries the 2 N M 128 contraction
    hipEvent_t evS1[2];
    const bool tS1 = prof_reserve(c, K_MATCH_SWEEP1, work, evS1);
    ProfScope ps(c, K_MATCH, work);
    launch_match_batch(s, nl, pd1, pn1, pd2, pn2, ppos, sqminratio, contrDistSq, nn, prow, pwork, tS1 ? evS1 : nullptr, trainPack ? ppack : nullptr);
  }
  if (db) {
    int *psel[MATCH_MAXB], *pddb[MATCH_MAXB];
    for (int k = 0; k < nl; k++) { psel[k] = (int *)((char *)c->dbSel.p + selOfs[k]); pddb[k] = (int *)((char *)c->matchRows.p + ddbOfs[k]); }
    launch_db_select(s, nl, prow, pn1, nn, sqminratio >= 1.0, psel, (int *)c->dbSel.p, pddb);
    ProfScope ps(c, K_MATCH_DB, 0);      // its work, 2 x selected x rows x 128, is known once the rows are down
    launch_dbnn_min(s, nl, pd1, pn1, psel, (int *)c->dbSel.p, pddb, *db);
  }
  MX_HIP(ctx_copy(c, hrow, c->matchRows.p, rowB, hipMemcpyDeviceToHost));
  MX_HIP(ctx_sync(c));
  MX_HIP(hipGetLastError());
  for (int k = 0; k < nl; k++) {
    const int *ddb = db ? (const int *)(hrow + ddbOfs[k]) : nullptr;
    rows_to_tentatives((const MatchRow *)(hrow + rowOfs[k]), pn1[k], nn, out[live[k]], ddb, sqminratio, d2byDB ? &d2byDB[live[k]] : nullptr);
    if (db && c->prof.enabled) {
      long sel = 0;
      for (int q = 0; q < pn1[k]; q++) sel += ddb[q] != 0x7fffffff;
      c->prof.work[K_MATCH_DB] += 2.0 * (double)sel * (double)db->rows * 128;
    }
  }
  return MODSX_OK;
}

int match_device(modsx_ctx *c, const uint8_t *d1, int n1, const uint8_t *d2, int n2, const double *pos2Host,
                 double ratioT, double contradDist, int nn, std::vector<modsx_tentative> &out, const DbSet *db, std::vector<double> *d2byDB) {
  return match_device_batch(c, 1, &d1, &n1, &d2, &n2, &pos2Host, ratioT, contradDist, nn, &out, nullptr, nullptr, db, d2byDB);
}

// The matcher computes on u8: the reference's SIFT-family descriptors hold the integers 0..255
// ((int)(512 v + 0.5) clamped, siftdesc.cpp:218-274).  Anything else (fractions, values out of range, NaN) would be
// matched with different distances than FLANN's float L2, so it is refused instead of being truncated silently.
bool desc_f32_to_u8(const float *f, size_t n, uint8_t *u) {
  bool ok = true;
  for (size_t i = 0; i < n; i++) {
    const float v = f[i];
    const int b = (v >= 0.f && v <= 255.f) ? (int)v : -1;
    ok = ok && b >= 0 && (float)b == v;
    u[i] = (uint8_t)(b < 0 ? 0 : b);
  }
  return ok;
}

int match_host_desc(modsx_ctx *c, const float *desc1, int n1, const float *desc2, int n2, const double *pos2,
                    double ratioT, double contradDist, int nn, std::vector<modsx_tentative> &out, const DbSet *db, std::vector<double> *d2byDB) {
  out.clear();
  if (d2byDB) d2byDB->clear();
  if (n1 == 0 || n2 == 0) return MODSX_OK;
  std::vector<uint8_t> u1((size_t)n1 * 128), u2((size_t)n2 * 128);
  if (!desc_f32_to_u8(desc1, u1.size(), u1.data()) || !desc_f32_to_u8(desc2, u2.size(), u2.data())) {
    set_error("modsx_match_fginn: descriptors must hold the integers 0..255 (SIFT-family quantisation)");
    return MODSX_ERR_ARG;
  }
  if (!c->descU8[0].ensure(u1.size()) || !c->descU8[1].ensure(u2.size())) return MODSX_ERR_NOMEM;
  MX_HIP(hipMemcpyAsync(c->descU8[0].p, u1.data(), u1.size(), hipMemcpyHostToDevice, c->stream));
  MX_HIP(hipMemcpyAsync(c->descU8[1].p, u2.data(), u2.size(), hipMemcpyHostToDevice, c->stream));
  MX_HIP(hipStreamSynchronize(c->stream));
  return match_device(c, (uint8_t *)c->descU8[0].p, n1, (uint8_t *)c->descU8[1].p, n2, pos2, ratioT, contradDist, nn, out, db, d2byDB);
}

// ---- the descriptor database of MatchFlannFGINNPlusDB (cv::Mat descDB of mods.cpp:207-216) ---------------------------------------
// rows: n x 128 values, u8 (dtype 0) or f32 holding the integers 0..255 (dtype 1).  The host validates, finds the parity class of
// every row (c = |b'|^2 + 2 sum b' is odd iff sum b is) and hands k_db_pack the first slot of every 256-row workgroup in each class.
DbSet *db_create(modsx_ctx *c, const void *rows, long n, int dtype) {
  if (!rows || n < 1 || (dtype != 0 && dtype != 1)) { set_error("modsx_db_create: bad argument (n >= 1 rows of 128 values, dtype 0 = u8 / 1 = f32)"); return nullptr; }
  if (n > MODSX_DB_MAX_ROWS) { set_error("modsx_db_create: more than MODSX_DB_MAX_ROWS rows"); return nullptr; }
  CtxBusy busy(c);
  std::vector<uint8_t> conv;
  const uint8_t *u8 = (const uint8_t *)rows;
  if (dtype == 1) {
    conv.resize((size_t)n * 128);
    if (!desc_f32_to_u8((const float *)rows, conv.size(), conv.data())) {
      set_error("modsx_db_create: descriptors must hold the integers 0..255 (SIFT-family quantisation)");
      return nullptr;
    }
    u8 = conv.data();
  }
  const int nblk = db_pack_blocks(n);
  std::vector<int2> base((size_t)nblk);
  std::vector<unsigned char> odd((size_t)n);
  long nOdd = 0;
  for (long i = 0; i < n; i++) {
    unsigned sum = 0;
    for (int k = 0; k < 128; k++) sum += u8[(size_t)i * 128 + k];
    odd[i] = sum & 1; nOdd += sum & 1;
  }
  const DbGeo geo = db_geo(n, nOdd);
  int e = 0, o = geo.TEp * 32;
  for (int b = 0; b < nblk; b++) {
    base[b] = make_int2(e, o);
    const long hi = std::min(n, (long)(b + 1) * 256);
    for (long i = (long)b * 256; i < hi; i++) { if (odd[i]) o++; else e++; }
  }
  DbSet *db = new DbSet();
  db->dev = c->dev; db->rows = n; db->geo = geo;
  const size_t tilesB = db_tiles_bytes(geo), hrowB = db_hrow_bytes(geo);
  DevBuf raw, dbase;
  bool ok = db->store.ensure(tilesB + hrowB) && raw.ensure((size_t)n * 128) && dbase.ensure((size_t)nblk * sizeof(int2));
  if (ok) {
    db->tiles = (const unsigned char *)db->store.p; db->hrow = (const int *)((char *)db->store.p + tilesB);
    ok = hipMemcpyAsync(raw.p, u8, (size_t)n * 128, hipMemcpyHostToDevice, c->stream) == hipSuccess &&
         hipMemcpyAsync(dbase.p, base.data(), (size_t)nblk * sizeof(int2), hipMemcpyHostToDevice, c->stream) == hipSuccess;
    if (ok) {
      launch_db_pack(c->stream, (const uint8_t *)raw.p, n, (const int2 *)dbase.p, nOdd, geo, (unsigned char *)db->store.p, (int *)((char *)db->store.p + tilesB));
      ok = hipStreamSynchronize(c->stream) == hipSuccess && hipGetLastError() == hipSuccess;
    }
    if (!ok) set_error("modsx_db_create: upload or packing failed");
  }
  raw.release(); dbase.release();
  if (!ok) { db->store.release(); delete db; return nullptr; }
  return db;
}
void db_free(DbSet *db) {
  if (!db) return;
  db->store.release();
  delete db;
}
// stage tap: squared L2 distance of every query to its nearest database row (every query is "selected")
int db_nearest(modsx_ctx *c, const DbSet &db, const float *desc, int n, float *dmin) {
  CtxBusy busy(c);
  if (db.dev != c->dev) { set_error("modsx_db_nearest: the descriptor database lives on another device"); return MODSX_ERR_ARG; }
  if (n == 0) return MODSX_OK;
  std::vector<uint8_t> u((size_t)n * 128);
  if (!desc_f32_to_u8(desc, u.size(), u.data())) {
    set_error("modsx_db_nearest: descriptors must hold the integers 0..255 (SIFT-family quantisation)");
    return MODSX_ERR_ARG;
  }
  const size_t nB = align_up((size_t)n * 4, 256);
  if (!c->descU8[0].ensure(u.size()) || !c->dbSel.ensure(256 + nB) || !c->matchRows.ensure(nB)) return MODSX_ERR_NOMEM;
  MX_HIP(hipMemcpyAsync(c->descU8[0].p, u.data(), u.size(), hipMemcpyHostToDevice, c->stream));
  const uint8_t *d1 = (const uint8_t *)c->descU8[0].p;
  int *sel = (int *)((char *)c->dbSel.p + 256), *cnt = (int *)c->dbSel.p, *dd = (int *)c->matchRows.p;
  launch_db_select(c->stream, 1, nullptr, &n, 2, true, &sel, cnt, &dd);
  {
    ProfScope ps(c, K_MATCH_DB, 2.0 * n * (double)db.rows * 128);
    launch_dbnn_min(c->stream, 1, &d1, &n, &sel, cnt, &dd, db);
  }
  std::vector<int> h((size_t)n);
  MX_HIP(hipMemcpyAsync(h.data(), dd, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  MX_HIP(hipStreamSynchronize(c->stream));
  MX_HIP(hipGetLastError());
  for (int i = 0; i < n; i++) dmin[i] = (float)h[i];
  return MODSX_OK;
}

// ------------------------------------------------------------------------------------------------
// one step of the mods.cpp loop for an identity view
// ------------------------------------------------------------------------------------------------
// DuplicateFiltering + LORANSACFiltering on the tentatives of one pair (mods.cpp:300-342, doBeforeRANSAC = 1).
// Fills the counters, H and the three malloc'd arrays of `res` (which must not own arrays yet).
void verify_tentatives(const std::vector<modsx_region> &r1, const std::vector<modsx_region> &r2,
                       const std::vector<modsx_tentative> &tents, const modsx_pair_params &pp, modsx_pair_result *res) {
  RegList a, b;
  a.add(r1); b.add(r2);
  verify_tentatives(a, b, tents, pp, res);
}
// kp1(i) / kp2(i): the seven doubles x, y, a11, a12, a21, a22, s of region i's reproj_kp -- all that DuplicateFiltering and
// LO-RANSAC read of a region
template <class K1, class K2>
static void verify_core(const K1 &kp1, const K2 &kp2, const std::vector<modsx_tentative> &tents, const modsx_pair_params &pp,
                        modsx_pair_result *res) {
  HostMark hm;
  res->n_tentatives = (int)tents.size();
  const int T0 = (int)tents.size();
  std::vector<double> pts((size_t)T0 * 4 + 4), key(T0 + 1);
  for (int i = 0; i < T0; i++) {
    const double *a = kp1(tents[i].q), *b = kp2(tents[i].t0);
    pts[4 * i] = a[0]; pts[4 * i + 1] = a[1]; pts[4 * i + 2] = b[0]; pts[4 * i + 3] = b[1];
    key[i] = tents[i].ratio;
  }
  hm.mark("verify: points");
  std::vector<int> order(T0 + 1);
  std::vector<unsigned char> keepd(T0 + 1);
  duplicate_filtering(pts.data(), key.data(), T0, pp.duplicateDist, 1, order.data(), keepd.data());
  hm.mark("verify: duplicate filter");
  std::vector<modsx_tentative> uniq;
  for (int i = 0; i < T0; i++) if (keepd[i]) uniq.push_back(tents[order[i]]);
  const int T = (int)uniq.size();
  res->n_unique = T;
  std::vector<double> p2((size_t)T * 4 + 4), l1((size_t)T * 5 + 5), l2((size_t)T * 5 + 5);
  for (int i = 0; i < T; i++) {
    const double *a = kp1(uniq[i].q), *b = kp2(uniq[i].t0);
    p2[4 * i] = a[0]; p2[4 * i + 1] = a[1]; p2[4 * i + 2] = b[0]; p2[4 * i + 3] = b[1];
    for (int k = 0; k < 5; k++) { l1[5 * i + k] = a[2 + k]; l2[5 * i + k] = b[2 + k]; }
  }
  res->tentatives = (modsx_tentative *)malloc(sizeof(modsx_tentative) * std::max(1, T));
  res->ransac_inlier = (unsigned char *)calloc(std::max(1, T), 1);
  res->verified = (unsigned char *)calloc(std::max(1, T), 1);
  for (int i = 0; i < T; i++) res->tentatives[i] = uniq[i];
  hm.mark("verify: unique lists");
  double Hraw[9];
  int dout[3] = {0, 0, 0};
  int nv;
  if (pp.useF)
    nv = loransac_f(p2.data(), l1.data(), l2.data(), T, pp.err_threshold, pp.confidence, pp.max_samples,
                    pp.localOptimization, pp.LAFCoef, pp.doSymmCheck, pp.errorType, pp.ransac_seed, res->H,
                    res->ransac_inlier, res->verified, dout);
  else
    nv = loransac_h(p2.data(), l1.data(), l2.data(), T, pp.err_threshold, pp.confidence, pp.max_samples,
                    pp.localOptimization, pp.HLAFCoef, pp.doSymmCheck, pp.ransac_seed, res->H, Hraw, res->ransac_inlier,
                    res->verified, dout, pp.errorType);
  hm.mark("verify: lo-ransac + checks");
  res->n_verified = nv < 0 ? 0 : nv;
  res->n_ransac_inliers = 0;
  for (int i = 0; i < T; i++) res->n_ransac_inliers += res->ransac_inlier[i];
  res->ransac_samples = dout[0]; res->ransac_lo = dout[1];
}

void verify_tentatives(const RegList &r1, const RegList &r2, const std::vector<modsx_tentative> &tents,
                       const modsx_pair_params &pp, modsx_pair_result *res) {
  static_assert(offsetof(modsx_keypoint, x) == 0 && offsetof(modsx_keypoint, s) == 48, "x, y, a11, a12, a21, a22, s are seven consecutive doubles");
  verify_core([&](size_t i) { return &r1[i].reproj_kp.x; }, [&](size_t i) { return &r2[i].reproj_kp.x; }, tents, pp, res);
}
// The same on geometry rows (kp[7 i ..]: what the view-sharded pair call moves instead of whole regions).  The list of a step with
// several descriptor classes repeats its n regions once per class (index = class * n + region), as the RegList of such a step does.
void verify_tentatives_kp(const double *kp1, size_t n1, const double *kp2, size_t n2, const std::vector<modsx_tentative> &tents,
                          const modsx_pair_params &pp, modsx_pair_result *res) {
  verify_core([&](size_t i) { return kp1 + 7 * (n1 ? i % n1 : 0); }, [&](size_t i) { return kp2 + 7 * (n2 ? i % n2 : 0); }, tents, pp, res);
}

// One step of mods.cpp's loop (identity view) for G <= MAXB / 2 independent pairs at once: the 2G images go through
// detection, orientation and description as ONE batch (one launch set, blockIdx.z / job tables select the image), then
// each pair is matched and verified.  Results are those of G separate calls.
int match_pair_group(modsx_ctx *c, const modsx_image *const *imgs1, const modsx_image *const *imgs2, int G,
                     const modsx_pair_params &pp, modsx_pair_result *res, std::vector<VerifyTask> *deferred) {
  CtxBusy busy(c);
  if (G < 1 || G > PAIR_GROUP || 2 * G > MAXB) { set_error("match_pair_group: group size"); return MODSX_ERR_ARG; }
  for (int g = 0; g < G; g++) {
    memset(&res[g], 0, sizeof res[g]);
    for (int i = 0; i < 9; i++) res[g].H[i] = -1;
  }
  const int n = 2 * G;
  const modsx_image *imgs[MAXB];
  for (int g = 0; g < G; g++) { imgs[2 * g] = imgs1[g]; imgs[2 * g + 1] = imgs2[g]; }
  struct SetScope { SetScope() { host_set_enter(); } ~SetScope() { host_set_leave(); } } setScope;   // a launch set in flight (host pool policy)
  const double t0 = now_ms();
  std::vector<modsx_keypoint> kps[MAXB];
  int rc = detect_keypoints_batch(c, imgs, n, pp.det, nullptr, nullptr, kps);
  if (rc) return rc;
  std::vector<modsx_region> regs[MAXB], oriented[MAXB];
  for (int i = 0; i < n; i++) {
    regs[i].resize(kps[i].size());
    detect_affine_regions(kps[i].data(), (int)kps[i].size(), 0, MODSX_DET_HESSIAN, regs[i].data());
  }
  const double t1 = now_ms();
  // the step's descriptor classes: ONE oriented list (Half-folded orientation histogram iff a Half type is among them,
  // imagerepresentation.cpp:693-706, 1259-1264, 1288-1296), one pass over the patches for all of them
  DescSet ds;
  rc = resolve_descs(pp, nullptr, ds);
  if (rc) return rc;
  const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  OriReproj rp[MAXB];     // the reprojection below: identity, the image's own size
  for (int i = 0; i < n; i++) rp[i] = {eye, imgs[i]->cols, imgs[i]->rows};
  rc = detect_orientation_batch(c, imgs, n, regs, pp.ori_mrSize, pp.ori_patchSize, ds.half() ? 1 : 0, pp.ori_maxAngles, pp.ori_threshold,
                                0, oriented, rp);
  if (rc) return rc;
  for (int i = 0; i < n; i++) {
    int m = reproject_regions(oriented[i].data(), (int)oriented[i].size(), eye, imgs[i]->cols, imgs[i]->rows);
    oriented[i].resize(m);
  }
  const double t2 = now_ms();
  rc = describe_batch(c, imgs, n, oriented, pp.desc_mrSize, pp.desc_patchSize, 0, pp.desc_photoNorm, ds.type[0],
                      pp.desc_maxBinValue, nullptr, nullptr, nullptr, &ds);
  if (rc) return rc;
  const double t3 = now_ms();
  double tMatch = 0, tVerify = 0;
  // classes in the order GetCorresponcesVector("All", "All") walks them: descriptor NAME order (correspondencebank.cpp:117-179)
  int ord[MODSX_MAX_DESC];
  desc_class_order(ds, ord);
  auto desc_of = [&](int k, int img) -> const uint8_t * { return (const uint8_t *)(k == 0 ? c->descU8[img].p : c->descU8x[k - 1][img].p); };
  std::vector<double> pos2v[MAXB / 2];
  std::vector<modsx_tentative> tentsv[MAXB / 2];
  const double m0 = now_ms();
  for (int g = 0; g < G; g++) {
    const std::vector<modsx_region> &rb = oriented[2 * g + 1];
    res[g].n_regions1 = (int)oriented[2 * g].size() * ds.n;
    res[g].n_regions2 = (int)rb.size() * ds.n;
    pos2v[g].resize(rb.size() * 2 + 2);
    for (size_t i = 0; i < rb.size(); i++) { pos2v[g][2 * i] = rb[i].reproj_kp.x; pos2v[g][2 * i + 1] = rb[i].reproj_kp.y; }
  }
  // the G matching problems of a class share the matcher's launches; each class has its own FGINN threshold
  for (int oi = 0; oi < ds.n; oi++) {
    const int k = ord[oi];
    const uint8_t *pd1[MAXB / 2], *pd2[MAXB / 2];
    const double *ppos[MAXB / 2];
    int pn1[MAXB / 2], pn2[MAXB / 2];
    std::vector<modsx_tentative> part[MAXB / 2];
    for (int g = 0; g < G; g++) {
      pd1[g] = desc_of(k, 2 * g); pd2[g] = desc_of(k, 2 * g + 1);
      pn1[g] = (int)oriented[2 * g].size(); pn2[g] = (int)oriented[2 * g + 1].size(); ppos[g] = pos2v[g].data();
    }
    for (int g0 = 0; g0 < G; g0 += MATCH_MAXB) {
      const int nbm = std::min(MATCH_MAXB, G - g0);
      rc = match_device_batch(c, nbm, pd1 + g0, pn1 + g0, pd2 + g0, pn2 + g0, ppos + g0, ds.ratio[k], pp.contradDist, pp.nn,
                              part + g0, nullptr, nullptr, fginn_db_for(c, ds.type[k]));
      if (rc) return rc;
    }
    for (int g = 0; g < G; g++) {
      const int o1 = oi * pn1[g], o2 = oi * pn2[g];
      if (oi == 0) { tentsv[g].swap(part[g]); continue; }
      for (modsx_tentative t : part[g]) {
        t.q += o1; t.t0 += o2;
        if (t.t1 >= 0) t.t1 += o2;
        if (t.tj >= 0) t.tj += o2;
        tentsv[g].push_back(t);
      }
    }
  }
  tMatch = now_ms() - m0;
  for (int g = 0; g < G; g++) {
    if (deferred) {   // modsx_match_pairs: verification is handed to the caller's helper threads
      deferred->emplace_back();
      VerifyTask &t = deferred->back();
      t.own.resize(2);
      t.own[0].swap(oriented[2 * g]); t.own[1].swap(oriented[2 * g + 1]);
      for (int oi = 0; oi < ds.n; oi++) { t.l1.add(t.own[0]); t.l2.add(t.own[1]); }
      t.tents.swap(tentsv[g]); t.res = &res[g]; t.dev = c->dev;
    } else {
      const double m1 = now_ms();
      RegList l1, l2;
      for (int oi = 0; oi < ds.n; oi++) { l1.add(oriented[2 * g]); l2.add(oriented[2 * g + 1]); }
      const int nr1 = res[g].n_regions1, nr2 = res[g].n_regions2;
      verify_tentatives(l1, l2, tentsv[g], pp, &res[g]);
      res[g].n_regions1 = nr1; res[g].n_regions2 = nr2;
      tVerify += now_ms() - m1;
    }
  }
  const double t5 = now_ms();
  prof_collect(c);
  // per-stage wall time of the group, divided by the number of pairs it carried
  c->timings[0] = (t1 - t0) / G; c->timings[1] = (t2 - t1) / G; c->timings[2] = (t3 - t2) / G; c->timings[3] = tMatch / G;
  c->timings[4] = tVerify / G; c->timings[5] = (t5 - t0) / G;
  return MODSX_OK;
}

int match_pair(modsx_ctx *c, const modsx_image *img1, const modsx_image *img2, const modsx_pair_params &pp,
               modsx_pair_result *res) {
  return match_pair_group(c, &img1, &img2, 1, pp, res);
}

}  // namespace mx
