// Library core: error reporting, the device binding, the device buffer cache, unicode tables and
// measurement hooks.  (The scan is cs_scan.hip, the column cs_column.hip, its metadata and the tile
// planners cs_plan.hip.)
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <unordered_map>

#include "_gen/unicode_tables.inc"  // cs_unicode_flags[65536], cs_charcases[65536]
#include "cs_internal.h"
#include "device_utils.h"
#include "tile_utils.h"

using namespace csdev;

namespace cs {

// ---------------------------------------------------------------- errors ----
static thread_local std::string g_last_error;
void set_last_error(const std::string& msg) { g_last_error = msg; }
void fail(int code, const std::string& msg) { throw Error{code, msg}; }

// ------------------------------------------------------------ device state --
// The pool's lock: the device binding, the block cache, the event pool and the known streams.  Never held together with
// g_prof_mu (below): no function takes both, and nothing called under either takes the other.
static std::mutex g_mu;
static int g_device = -1;
static uint8_t* g_d_flags = nullptr;
static uint16_t* g_d_cases = nullptr;
static int64_t g_in_use = 0;
// A cached block remembers the stream it was last used on and, once a second stream has been seen, an EVENT recorded on
// that stream when the block was released: a different stream that takes the block waits for the event on the device
// (hipStreamWaitEvent) -- the host does not wait, where a device-wide synchronisation per released block used to turn
// every op of a multi-stream caller into dozens of full stalls.
struct CachedBlock {
  void* first;
  hipStream_t second;
  std::vector<hipEvent_t> released;  // one per stream known at the release (a column made on one stream may have been read on another)
};
static std::multimap<size_t, CachedBlock> g_cache;  // capacity -> block
static int64_t g_cached_bytes = 0;                  // sum of the capacities in g_cache
static int64_t g_cache_limit = 0;                   // 0 = not sized yet (half the device's memory, CS_POOL_MAX_MB overrides)
static std::atomic<long long> g_mallocs{0};         // hipMalloc calls made by dev_alloc (cs_debug_malloc_count)
static const hipStream_t kNoStream = reinterpret_cast<hipStream_t>(~(uintptr_t)0);  // "last used by nobody we still know"
static std::vector<hipEvent_t> g_event_pool;
// Streams that have asked for buffers.  While there is one (the usual case) stream order alone
// makes the reuse of a released block safe.  With more, a block may still be read by a kernel on
// a stream other than the one it was allocated on when its last handle goes away, so a release
// then records an event on every known stream, and whoever takes the block next waits for them on the device.
static std::set<hipStream_t> g_streams;
static std::atomic<bool> g_multi_stream{false};
static std::atomic<long long> g_fallbacks{0};

void require_device() {
  if (g_device < 0) fail(CS_ERR_NO_DEVICE, "cs_init has not succeeded: no usable gfx950 device (there is no CPU fallback)");
  // hipSetDevice is per thread: a host thread other than the one that ran cs_init would launch on device 0
  static thread_local int bound = -1;
  if (bound != g_device) {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != g_device) CS_HIP(hipSetDevice(g_device));
    bound = g_device;
  }
}
int bound_device() { return g_device; }
thread_local const char* g_last_route = "";
void note_route(const char* route) { g_last_route = route; }
// the op ran on the column's pieces (cs_virtual.hip): the inner launch's route under a "pieces:" prefix
thread_local char g_route_text[64];
void note_route_pieces() {
  char inner[48];
  snprintf(inner, sizeof inner, "%s", g_last_route);
  snprintf(g_route_text, sizeof g_route_text, "pieces:%s", inner);
  g_last_route = g_route_text;
}
// the scan put the rows with bytes >= 0x80 off to a second launch (regex_stream.h: ScanStreamArgs::deferred)
void note_route_put_off() {
  char inner[48];
  snprintf(inner, sizeof inner, "%s", g_last_route);
  snprintf(g_route_text, sizeof g_route_text, "%s+later", inner);
  g_last_route = g_route_text;
}
void note_fallback(const char* what) {
  if (g_fallbacks.fetch_add(1) == 0 || cs::cfg("CS_LOG_FALLBACKS"))
    fprintf(stderr, "custrings_amd: %s: the single-pass kernel gave up, recomputing with the two-pass kernels\n", what);
}
const uint8_t* d_unicode_flags() { return g_d_flags; }
const uint16_t* d_charcases() { return g_d_cases; }
const uint8_t* h_unicode_flags() { return cs_unicode_flags; }
const uint16_t* h_charcases() { return cs_charcases; }
int64_t dev_bytes_in_use() { return g_in_use; }

static void release_cache_locked() {
  for (auto& kv : g_cache) {
    (void)hipFree(kv.second.first);
    for (hipEvent_t e : kv.second.released) g_event_pool.push_back(e);
  }
  g_cache.clear();
  g_cached_bytes = 0;
}

// Capacity a new block gets for a request of `want` bytes (reference: the RMM pool behind every device_alloc,
// cpp/src/util.inl:90-106, python/tests/utils.py:25-34 -- a column a few KB larger than the last one must not cost a
// hipMalloc of gigabytes, 120-134 ms on this machine).  From 1 MiB on: 1/32 of headroom, then the next of eight
// geometric steps per octave, so the block also serves every later request up to 3 % larger (and, by the reuse rule in
// dev_alloc, down to 20 % smaller); at most 16 % over the request.  Below that the sizes of a pipeline's buffers vary
// more from column to column (a split column that few rows reach: +-10 %) and their bytes do not matter: 1/8 of headroom
// and four steps per octave from 4 KiB on, whole 4 KiB pages below.
static size_t size_class(size_t want) {
  if (want <= 4096) return 4096;
  const bool small = want < ((size_t)1 << 20);
  const size_t w = want + want / (small ? 8 : 32);
  const int e = 63 - __builtin_clzll((unsigned long long)w);
  const size_t step = (size_t)1 << (e - (small ? 2 : 3));
  return (w + step - 1) / step * step;
}
// the largest idle block a request may take: half as much again (one class up from the block a request 3 % larger was
// given: with 25 % a request for 15.06 MB missed an idle 18.87 MB block by 50 KB -- tools/pool_replay.py replays a trace of
// the pool's requests through this policy), or 256 KiB (the small blocks' classes are coarse)
static size_t reuse_limit(size_t want) { return want + std::max<size_t>(want / 2 + 4096, (size_t)256 << 10); }
constexpr int kPageBlocksAtFirstTouch = 64;  // page-sized blocks allocated together the first time one is needed (below)

// The cache is bounded: beyond the limit the largest idle blocks go back to the driver (hipFree waits for the device:
// rare by construction -- the limit is half the device's memory unless CS_POOL_MAX_MB says otherwise).
static void trim_cache_locked() {
  if (g_cache_limit == 0) {
    size_t free_b = 0, total_b = 0;
    if (const char* e = cs::cfg("CS_POOL_MAX_MB")) g_cache_limit = std::max<int64_t>(1, atoll(e)) << 20;
    else if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b) g_cache_limit = (int64_t)(total_b / 2);
    else g_cache_limit = (int64_t)64 << 30;
  }
  while (g_cached_bytes > g_cache_limit && !g_cache.empty()) {
    auto it = std::prev(g_cache.end());
    (void)hipFree(it->second.first);
    for (hipEvent_t e : it->second.released) g_event_pool.push_back(e);
    g_cached_bytes -= (int64_t)it->first;
    g_cache.erase(it);
  }
}

DevBuf::~DevBuf() {
  if (ipc_mapped && p) {
    (void)hipIpcCloseMemHandle(p);
    return;
  }
  if (!capacity || !p) return;
  std::vector<hipEvent_t> evs;
  if (g_multi_stream.load(std::memory_order_relaxed)) {
    std::vector<hipStream_t> streams;
    {
      std::lock_guard<std::mutex> lk(g_mu);
      streams.assign(g_streams.begin(), g_streams.end());
      while (evs.size() < streams.size() && !g_event_pool.empty()) {
        evs.push_back(g_event_pool.back());
        g_event_pool.pop_back();
      }
    }
    bool ok = true;
    while (ok && evs.size() < streams.size()) {
      hipEvent_t e = nullptr;
      ok = hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
      if (ok) evs.push_back(e);
    }
    std::vector<hipStream_t> dead;
    for (size_t i = 0; ok && i < streams.size(); ++i)
      if (hipEventRecord(evs[i], streams[i]) != hipSuccess) {  // (a stream its owner destroyed: forget it)
        (void)hipGetLastError();
        dead.push_back(streams[i]);
        ok = false;
      }
    if (!ok) {
      (void)hipDeviceSynchronize();  // (no complete set of events to wait for: the block is idle before anyone else may take it)
      std::lock_guard<std::mutex> lk(g_mu);
      for (hipEvent_t e : evs) g_event_pool.push_back(e);
      for (hipStream_t d : dead) g_streams.erase(d);
      evs.clear();
    }
  }
  std::lock_guard<std::mutex> lk(g_mu);
  g_in_use -= (int64_t)capacity;
  if (cs::cfg_int("CS_POOL_TRACE", 0) >= 2) fprintf(stderr, "pool- %zu %zu\n", bytes, capacity);
  g_cache.emplace(capacity, CachedBlock{p, stream, std::move(evs)});
  g_cached_bytes += (int64_t)capacity;
  trim_cache_locked();
}

Buf dev_alloc(size_t bytes, hipStream_t stream) {
  require_device();
  size_t want = ((bytes + 64 + 511) / 512) * 512;
  auto b = std::make_shared<DevBuf>();
  b->bytes = bytes;
  b->stream = stream;
  bool reused = false;
  hipStream_t prev = nullptr;
  std::vector<hipEvent_t> released;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_streams.insert(stream).second && g_streams.size() > 1) g_multi_stream.store(true);
    auto it = g_cache.lower_bound(want);
    if (it != g_cache.end() && it->first <= reuse_limit(want)) {
      b->p = it->second.first;
      b->capacity = it->first;
      prev = it->second.second;
      // (a block whose last stream is no longer known -- cs_stream_forget synchronised it, its owner may have destroyed
      // it since -- is idle: nothing to wait for, and the handle must not be touched)
      if (prev != stream && !g_streams.count(prev)) prev = stream;
      released = std::move(it->second.released);
      g_cache.erase(it);
      g_cached_bytes -= (int64_t)b->capacity;
      g_in_use += (int64_t)b->capacity;
      reused = true;
    }
  }
  if (cs::cfg_int("CS_POOL_TRACE", 0) >= 2) fprintf(stderr, "pool+ %zu %zu %s\n", bytes, reused ? b->capacity : (size_t)0, reused ? "hit" : "miss");
  if (reused) {
    // a block last used on another stream may still be in flight there: this stream waits for the release event on the
    // device (blocks released before a second stream existed carry none: the host waits for their stream once)
    if (!released.empty()) {
      struct BackToPool {  // (also when a wait below throws: the events are not lost)
        std::vector<hipEvent_t>& evs;
        ~BackToPool() {
          std::lock_guard<std::mutex> lk(g_mu);
          for (hipEvent_t e : evs) g_event_pool.push_back(e);
        }
      } back{released};
      for (hipEvent_t e : released) CS_HIP(hipStreamWaitEvent(stream, e, 0));
    } else if (prev != stream) {
      CS_HIP(hipStreamSynchronize(prev));
    }
    return b;
  }
  void* p = nullptr;
  const size_t asked = want;
  want = size_class(want);
  g_mallocs.fetch_add(1, std::memory_order_relaxed);
  if (cs::cfg("CS_POOL_TRACE")) {  // (tests / tools: which requests miss the pool)
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_cache.lower_bound(asked);
    fprintf(stderr, "custrings_amd pool: hipMalloc %zu bytes for a request of %zu (%zu idle blocks, %lld bytes; the next larger idle block: %zu)\n", want, asked, g_cache.size(),
            (long long)g_cached_bytes, it == g_cache.end() ? (size_t)0 : it->first);
  }
  hipError_t e = hipMalloc(&p, want);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    {
      std::lock_guard<std::mutex> lk(g_mu);
      (void)hipDeviceSynchronize();
      release_cache_locked();
    }
    e = hipMalloc(&p, want);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      fail(CS_ERR_ALLOC, "allocate error: " + std::to_string(want) + " bytes (" + hipGetErrorString(e) + ")");
    }
  }
  b->p = p;
  b->capacity = want;
  std::lock_guard<std::mutex> lk(g_mu);
  g_in_use += (int64_t)want;
  // Page-sized blocks (scalars, flags, the chars of a column that few rows reach): how many of them are live at once
  // varies from column to column as sizes cross the page -- the first one brings its siblings along (each its own
  // allocation: any of them may later be exported over HIP IPC), so that a later op does not stop for a 4 KB hipMalloc.
  static bool page_blocks_made = false;
  if (want == 4096 && !page_blocks_made) {
    page_blocks_made = true;
    for (int i = 0; i < kPageBlocksAtFirstTouch; ++i) {
      void* q = nullptr;
      if (hipMalloc(&q, 4096) != hipSuccess) {
        (void)hipGetLastError();
        break;
      }
      g_mallocs.fetch_add(1, std::memory_order_relaxed);
      g_cache.emplace((size_t)4096, CachedBlock{q, kNoStream, {}});
      g_cached_bytes += 4096;
    }
  }
  return b;
}

Buf dev_wrap(const void* p, size_t bytes) {
  auto b = std::make_shared<DevBuf>();
  b->p = const_cast<void*>(p);
  b->bytes = bytes;
  b->capacity = 0;
  b->borrowed = true;
  return b;
}

Buf dev_owned(const Buf& b, hipStream_t s) {
  if (!b || !b->borrowed) return b;
  Buf own = dev_alloc(b->bytes, s);
  if (b->bytes) {
    CS_HIP(hipMemcpyAsync(own->p, b->p, b->bytes, hipMemcpyDeviceToDevice, s));
    CS_HIP(hipStreamSynchronize(s));
  }
  return own;
}

void* pinned_scratch(size_t bytes) {
  static thread_local void* p = nullptr;
  static thread_local size_t cap = 0;
  if (bytes > cap) {
    if (p) (void)hipHostFree(p);
    size_t want = bytes < 4096 ? 4096 : bytes;
    CS_HIP(hipHostMalloc(&p, want, hipHostMallocDefault));
    cap = want;
  }
  return p;
}

// ------------------------------------------------------------- profiling ----
struct ProfEntry {
  double ms = 0;
  int64_t launches = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};
// The profiler's lock: g_prof.  It is held while cs_prof_reset / cs_prof_get wait for their events, which stalls other
// ProfScopes only.  Never held together with g_mu (above): nothing below allocates from the pool.
static std::mutex g_prof_mu;
static std::atomic<bool> g_prof_on{false};
static std::unordered_map<std::string, ProfEntry> g_prof;

ProfScope::ProfScope(const char* nm, hipStream_t st) : name(nm), s(st) {
  if (!g_prof_on) return;
  (void)hipEventCreate(&a);
  (void)hipEventCreate(&b);
  (void)hipEventRecord(a, s);
}
ProfScope::~ProfScope() {
  if (!a) return;
  (void)hipEventRecord(b, s);
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof[name].pending.emplace_back(a, b);
}
static void prof_collect(ProfEntry& e) {
  for (auto& pr : e.pending) {
    (void)hipEventSynchronize(pr.second);
    float ms = 0;
    if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
      e.ms += ms;
      e.launches += 1;
    }
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  e.pending.clear();
}

Buf zeroed_count(hipStream_t s) {
  Buf acc = dev_alloc(8, s);
  CS_HIP(hipMemsetAsync(acc->p, 0, 8, s));
  return acc;
}
int64_t read_count(const Buf& acc, hipStream_t s) {
  int64_t* host = (int64_t*)pinned_scratch(8);
  CS_HIP(hipMemcpyAsync(host, acc->p, 8, hipMemcpyDeviceToHost, s));
  CS_HIP(hipStreamSynchronize(s));
  return host[0];
}
}  // namespace cs

using namespace cs;

// =============================================================== public ABI ==
extern "C" {

int cs_version(void) { return 100; }
int cs_has_experiments(void) {
#if defined(CS_EXPERIMENTS)
  return 1;
#else
  return 0;
#endif
}
const char* cs_last_error(void) { return g_last_error.c_str(); }

int cs_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int cs_init(int device) {
  return guard([&] {
    (void)cs::cfg("CS_DEVICE");  // (the CS_* switches are read from the environment here, once: cs_config.h)
    int n = cs_device_count();
    if (n <= 0) fail(CS_ERR_NO_DEVICE, "no HIP device visible (there is no CPU fallback)");
    if (device < 0 || device >= n) fail(CS_ERR_INVALID_ARG, "device index out of range");
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_device == device) {
      CS_HIP(hipSetDevice(device));
      return;
    }
    if (g_device >= 0) fail(CS_ERR_INVALID_ARG, "this process is already bound to another device (one process per GPU)");
    CS_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    CS_HIP(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
      fail(CS_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    CS_HIP(hipMalloc((void**)&g_d_flags, 65536));
    CS_HIP(hipMalloc((void**)&g_d_cases, 65536 * 2));
    CS_HIP(hipMemcpy(g_d_flags, cs_unicode_flags, 65536, hipMemcpyHostToDevice));
    CS_HIP(hipMemcpy(g_d_cases, cs_charcases, 65536 * 2, hipMemcpyHostToDevice));
    g_device = device;
  });
}

int cs_current_device(void) { return g_device; }
int64_t cs_fallback_count(void) { return (int64_t)g_fallbacks.load(); }
const char* cs_debug_last_route(void) { return cs::g_last_route; }
int cs_config_set(const char* name, const char* value) {
  return guard([&] {
    if (!name || std::strncmp(name, "CS_", 3) != 0) fail(CS_ERR_INVALID_ARG, "config: the switches are named CS_*");
    cs::cfg_set(name, value);
  });
}
int64_t cs_device_bytes_in_use(void) { return dev_bytes_in_use(); }
int64_t cs_debug_malloc_count(void) { return (int64_t)g_mallocs.load(); }
int64_t cs_pool_cached_bytes(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  return g_cached_bytes;
}
int cs_pool_trim(int64_t keep_bytes) {
  return guard([&] {
    require_device();
    CS_HIP(hipDeviceSynchronize());
    std::lock_guard<std::mutex> lk(g_mu);
    const int64_t limit = g_cache_limit;
    g_cache_limit = std::max<int64_t>(keep_bytes, 1);
    trim_cache_locked();
    g_cache_limit = limit;
  });
}
void cs_free(void* p) { free(p); }

int cs_prof_reset(void) {
  return guard([&] {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& kv : g_prof) prof_collect(kv.second);
    g_prof.clear();
  });
}
int cs_prof_enable(int on) {
  g_prof_on = on != 0;
  return CS_OK;
}
int cs_stream_forget(cs_stream stream) {
  return guard([&] {
    if (!stream) return;
    (void)hipStreamSynchronize(S(stream));  // (what it still runs on cached blocks is done before they can be handed out again)
    std::lock_guard<std::mutex> lk(g_mu);
    g_streams.erase(S(stream));
    // cached blocks that name the stream as their last user are idle now; the handle may be destroyed by its owner, so
    // nobody may synchronise it again: dev_alloc treats a block whose stream is not in g_streams as idle (blocks that
    // are released LATER with this stream in their DevBuf are covered by the same rule).  Their release events stay:
    // waiting for an event recorded on a destroyed stream is defined (it has completed).
    for (auto& kv : g_cache)
      if (kv.second.second == S(stream)) kv.second.second = kNoStream;
  });
}
__global__ void __launch_bounds__(256) k_debug_spin(unsigned long long ticks) {
  extern __shared__ uint32_t spin_lds[];
  if (threadIdx.x == 0) spin_lds[0] = 1;  // (the LDS is what keeps other workgroups off the CU)
  const unsigned long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}
int cs_debug_spin(int blocks, int lds_bytes, int milliseconds, cs_stream stream) {
  return guard([&] {
    if (blocks < 1 || lds_bytes < 4 || lds_bytes > 160 * 1024 || milliseconds < 0) fail(CS_ERR_INVALID_ARG, "debug_spin: bad arguments");
    require_device();
    if (lds_bytes > 48 * 1024)
      CS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_debug_spin), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    hipLaunchKernelGGL(k_debug_spin, dim3((unsigned)blocks), dim3(256), (size_t)lds_bytes, S(stream), (unsigned long long)milliseconds * 100000ull);  // (100 MHz)
    CS_HIP(hipGetLastError());
  });
}
int cs_prof_get(const char* kernel, double* total_ms, int64_t* launches) {
  return guard([&] {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    auto it = g_prof.find(kernel ? kernel : "");
    if (it == g_prof.end()) {
      if (total_ms) *total_ms = 0;
      if (launches) *launches = 0;
      return;
    }
    prof_collect(it->second);
    if (total_ms) *total_ms = it->second.ms;
    if (launches) *launches = it->second.launches;
  });
}

}  // extern "C"

