// Device memory of libmetamaps_hip (host side): the byte meter, pieces of pooled blocks, the per-device pool of index-scale blocks, the
// per-context cache, the one out-of-memory ladder, and DBuf.  Included by mm_common.hpp behind its error plumbing (mm::Error, MM_HIP).
// In reading order: switches and trace, meter, slabs, pool, DevAlloc (the cache), registry, reclaim, DevAlloc::get, DBuf.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include "mm_alloc_rules.hpp"
#include "mm_slab.hpp"
#include "mm_stream.hpp"

namespace mm {

// ---- device memory -----------------------------------------------------------------------------------
// Per-context caching allocator.  A batch needs dozens of temporaries; hipMalloc/hipFree synchronise the
// device, and ROCm 7.2's stream-ordered pool (hipMallocAsync) gave wrong results here when the library ran
// on the system HIP runtime (it only behaved under the older runtime that PyTorch bundles), so blocks are
// recycled by hand: a context owns ONE stream, every kernel and copy is issued on it, and a freed block
// handed to a later allocation is therefore only touched by work that is stream-ordered after its previous
// user.  Index-scale buffers (>= 8 GiB) bypass the cache.

// The allocator's switches, read once (the table: mm_env.hpp).
struct AllocEnv {
  // every block that comes from the driver, with its cost
  const bool trace = getenv("MM_ALLOC_TRACE") != nullptr;
  // off (MM_NO_POOL_RESCUE=1): no size classes, a request the driver refuses is not served from the pool, the whole pool goes back to the driver
  // when memory is short and before a device-filling build (mm_index.hip)
  const bool rescue = getenv("MM_NO_POOL_RESCUE") == nullptr;
  const bool slabs = getenv("MM_NO_SLABS") == nullptr;
  // blocks from this size on are "index-scale": pooled per device, not cached per context (MM_INDEX_SCALE_MB: test hook — with a few MB the pool,
  // and the slabs cut from it, come into play on a reference of a few Mbp)
  const size_t index_scale = [] { const char* e = getenv("MM_INDEX_SCALE_MB"); return e && atoll(e) > 0 ? (size_t)atoll(e) << 20 : (size_t)8 << 30; }();
  // MM_DEVICE_BYTES_CAP=<bytes> (a TEST HOOK) makes the library behave as if every device had only that much memory: dev_malloc fails with
  // hipErrorOutOfMemory beyond it and dev_mem_info reports it — the CLI's resident / sharded / streamed decision and the allocator's
  // out-of-memory paths are then exercised on a small input (tests/test_gpu_cli.py) instead of on a reference larger than 288 GB.
  const long long cap = [] { const char* e = getenv("MM_DEVICE_BYTES_CAP"); return e ? atoll(e) : 0; }();
};
inline const AllocEnv& alloc_env() { static const AllocEnv e; return e; }
// MM_ALLOC_TRACE=1: one line on stderr (tests/test_gpu_cli.py and tools/alloc_*.sh parse them)
__attribute__((format(printf, 1, 2))) inline void alloc_trace(const char* fmt, ...) {
  if (!alloc_env().trace) return;
  va_list ap; va_start(ap, fmt);
  fputs("MM_ALLOC_TRACE ", stderr); vfprintf(stderr, fmt, ap);
  va_end(ap);
}
using TraceClock = std::chrono::steady_clock;
inline double ms_since(TraceClock::time_point t0) { return std::chrono::duration<double, std::milli>(TraceClock::now() - t0).count(); }
inline double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::system_clock::now().time_since_epoch()).count(); }

// ---- meter: every device block of the library comes from dev_malloc and goes back through dev_free, so that the bytes it holds per device are known
struct DevMeter {
  std::atomic<long long> used[64];
  DevMeter() { for (auto& u : used) u = 0; }
};
inline DevMeter& dev_meter() { static DevMeter m; return m; }
inline int dev_current() { int d = 0; (void)hipGetDevice(&d); return d < 0 || d >= 64 ? 0 : d; }
inline hipError_t dev_malloc(void** p, size_t bytes) {
  DevMeter& m = dev_meter();
  const long long cap = alloc_env().cap;
  const int d = dev_current();
  if (cap > 0 && m.used[d].load() + (long long)bytes > cap) { *p = nullptr; return hipErrorOutOfMemory; }
  const hipError_t e = hipMalloc(p, bytes);
  if (e == hipSuccess) m.used[d] += (long long)bytes;
  return e;
}
// (SlabSet: mm_slab.hpp)
inline SlabSet& slab_set() { static SlabSet s; return s; }
inline void dev_free(void* p, size_t bytes) {
  if (!p) return;
  if (slab_set().give_back(p, bytes)) return;                    // (a piece of a pooled block: the block stays the device's)
  // the bytes go off the account of the device the block LIVES on (hipMalloc charged the device current at that time): the thread that frees —
  // a context's destructor on the CLI's main thread, another context trimming this one's cache — may have any device current
  int d = dev_current();
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) == hipSuccess && at.device >= 0 && at.device < 64) d = at.device; else (void)hipGetLastError();
  dev_meter().used[d] -= (long long)bytes; (void)hipFree(p);
}
inline hipError_t dev_mem_info(size_t* fr, size_t* tot) {
  const hipError_t e = hipMemGetInfo(fr, tot);
  const long long cap = alloc_env().cap;
  if (e == hipSuccess && cap > 0) {
    const long long left = std::max(0LL, cap - dev_meter().used[dev_current()].load());
    *tot = std::min<size_t>(*tot, (size_t)cap); *fr = std::min<size_t>(*fr, (size_t)left);
  }
  return e;
}
inline std::string oom_text(size_t want, hipError_t e) {         // what the device looks like when an allocation fails for good
  size_t fr = 0, tot = 0; (void)dev_mem_info(&fr, &tot);
  return std::string("hipMalloc of ") + std::to_string(want) + " bytes: " + hipGetErrorString(e) + " (device: " + std::to_string(fr >> 20) + " MiB free of " + std::to_string(tot >> 20) + ")";
}
[[noreturn]] inline void throw_alloc_failed(size_t want, hipError_t e) {
  (void)hipGetLastError();
  throw mm::Error(e == hipErrorOutOfMemory ? MM_ERR_NOMEM : MM_ERR_DEVICE, oom_text(want, e));
}

// ---- pool: index-scale blocks (>= 8 GiB) are recycled per device: on this runtime a freed block of that size is not free for long — one of the
// next allocations stalls for ~6 s (constant, whatever its own size; MM_ALLOC_TRACE) — and an index build, let alone a pass over
// the chunk indexes of a reference larger than HBM (built, mapped, dropped, chunk after chunk), frees and allocates tens of them.  A
// released block waits here for a request it fits (at most an eighth too large: index-scale blocks are what fills the device); everything is handed back to the driver when an
// allocation fails for lack of memory or the last context of the process goes.
struct BigPool {
  std::mutex m;
  std::multimap<size_t, void*> free_;
  size_t bytes = 0;
  void* take(size_t want, size_t* got) {
    std::lock_guard<std::mutex> lk(m);
    auto it = free_.lower_bound(want);
    if (it == free_.end() || !pool_block_fits(it->first, want)) return nullptr;
    void* p = it->second; *got = it->first; bytes -= it->first; free_.erase(it);
    return p;
  }
  void* take_at_least(size_t want, size_t* got) {               // the smallest pooled block that holds `want` (for a slab)
    std::lock_guard<std::mutex> lk(m);
    auto it = free_.lower_bound(want);
    if (it == free_.end()) return nullptr;
    void* p = it->second; *got = it->first; bytes -= it->first; free_.erase(it);
    return p;
  }
  void give(void* p, size_t sz) { std::lock_guard<std::mutex> lk(m); free_.emplace(sz, p); bytes += sz; }
  void trim() { std::lock_guard<std::mutex> lk(m); for (auto& kv : free_) dev_free(kv.second, kv.first); free_.clear(); bytes = 0; }
  // pooled blocks back to the driver, largest first, only until it can serve `need` bytes (what stays pooled is what the next chunk build takes
  // without a driver call; true: the driver now has the room)
  bool trim_until(size_t need) {
    std::lock_guard<std::mutex> lk(m);
    for (;;) {
      size_t fr = 0, tot = 0;
      if (dev_mem_info(&fr, &tot) == hipSuccess && fr >= need) return true;
      if (free_.empty()) return false;
      auto it = std::prev(free_.end());
      dev_free(it->second, it->first); bytes -= it->first; free_.erase(it);
    }
  }
};
inline BigPool& big_pool(int device) { static BigPool pools[64]; return pools[device < 0 || device >= 64 ? 0 : device]; }
inline size_t big_pool_bytes(int device) { return big_pool(device).bytes; }
inline void big_pool_adopt_idle(int device) {                    // slabs nothing is cut from any more are pooled blocks again
  for (auto& sl : slab_set().take_idle(device)) big_pool(device).give(sl.first, sl.second);
}
inline bool big_pool_trim_until(int device, size_t need) { big_pool_adopt_idle(device); return big_pool(device).trim_until(need); }
inline void big_pool_trim(int device) { big_pool_adopt_idle(device); big_pool(device).trim(); }   // (idle slabs go with the rest)
inline void* slab_piece(int device, size_t bytes) {              // a piece of a pooled index-scale block of the device, or nullptr
  if (void* p = slab_set().alloc(device, bytes)) return p;
  size_t got = 0;
  void* blk = big_pool(device).take_at_least(SlabSet::granules(bytes), &got);
  if (!blk) return nullptr;
  slab_set().adopt(device, blk, got);
  return slab_set().alloc(device, bytes);
}

// ---- the cache of one context
struct DevAlloc {
  hipStream_t stream = nullptr;
  int device = -1;                           // set by alloc_register
  std::mutex m;                              // the cache: its own context's thread, and any thread that trims it when the device is full
  // set for the duration of a device-filling index build (mm_index.hip): every index-scale allocation first hands the cached blocks back
  // and index-scale blocks go straight to and from the driver, so that the build's memory is returned WHILE it runs.  Returned in one
  // piece afterwards (~100 GB), it came back as a 1 s stall of a mapping step a few seconds later, twice in four bench runs (round 3).
  bool eager = false;
  bool in_build = false;                     // an index build runs on this context: its temporaries do not cut into pooled blocks the build itself is about to ask for
  std::multimap<size_t, void*> cache;        // size -> free block
  size_t cached_bytes = 0;
  void trim() {
    std::lock_guard<std::mutex> lk(m);
    if (cache.empty()) return;
    (void)mm::stream_sync(stream);
    for (auto& kv : cache) dev_free(kv.second, kv.first);
    cache.clear(); cached_bytes = 0;
  }
  // hands the largest cached blocks back to the driver until at most `keep` bytes stay cached (after an index build: its temporaries
  // are worth keeping for the next chunk's build, not a hundred gigabytes of them beside the mapping buffers of other contexts)
  void trim_to(size_t keep) {
    std::lock_guard<std::mutex> lk(m);
    if (cached_bytes <= keep) return;
    (void)mm::stream_sync(stream);
    while (cached_bytes > keep && !cache.empty()) { auto it = std::prev(cache.end()); dev_free(it->second, it->first); cached_bytes -= it->first; cache.erase(it); }
  }
  // A cached block serves a request it is at most 60 % too large for, and what comes from the driver (from 64 MiB on) is asked for a
  // quarter larger than needed: read batches differ (more or fewer seed hits, candidates, records), and on this runtime memory the
  // driver has seen freed is cleared when it is handed out again — 1 ms per 27 MB, up to seconds when a large region is due
  // (MM_ALLOC_TRACE, round 3: one 738 MB allocation of a bench step took 2.0 s).  With headroom the buffers of the first batches also
  // serve the later ones, and a process in steady state does not go to the driver at all.
  void* take_cached(size_t want, size_t* got) {
    std::lock_guard<std::mutex> lk(m);
    auto it = cache.lower_bound(want);
    if (it == cache.end() || !cache_fits(it->first, want)) return nullptr;
    void* p = it->second; *got = it->first; cached_bytes -= it->first; cache.erase(it);
    return p;
  }
  void* get(size_t bytes, size_t* got);      // (behind reclaim)
  void put(void* p, size_t bytes) { std::lock_guard<std::mutex> lk(m); cache.emplace(bytes, p); cached_bytes += bytes; }
  ~DevAlloc();
};

// ---- registry: free blocks cached by one context are memory another context of the same device may need (worker contexts beside the one that built
// the indexes): an allocation that fails for lack of memory asks every other context's cache to go back to the driver before it gives up.
struct AllocRegistry { std::mutex m; std::vector<DevAlloc*> v; };
inline AllocRegistry& alloc_registry() { static AllocRegistry r; return r; }
inline void alloc_register(DevAlloc* a, int device) { AllocRegistry& r = alloc_registry(); std::lock_guard<std::mutex> lk(r.m); a->device = device; r.v.push_back(a); }
// (a foreign thread is inside an allocator only while it holds the registry's lock: once this returns, none is or will be inside `a`)
inline void alloc_unregister(DevAlloc* a) {
  AllocRegistry& r = alloc_registry(); std::lock_guard<std::mutex> lk(r.m);
  for (size_t i = 0; i < r.v.size(); ++i) if (r.v[i] == a) { r.v.erase(r.v.begin() + (long)i); break; }
}
inline void alloc_trim_others(DevAlloc* self, int device) {      // (the caller holds no allocator lock)
  AllocRegistry& r = alloc_registry(); std::lock_guard<std::mutex> lk(r.m);
  for (DevAlloc* a : r.v) if (a != self && a->device == device) a->trim();
}
inline DevAlloc::~DevAlloc() { alloc_unregister(this); trim(); }
inline DevAlloc*& current_alloc() { static thread_local DevAlloc* a = nullptr; return a; }
inline hipStream_t& current_stream() { static thread_local hipStream_t s = nullptr; return s; }

// ---- out of memory
// A request the driver has refused for lack of memory, served from what the device's pool holds WITHOUT handing the pool back to the driver:
// the caches go back first (their pieces of pooled blocks return to the blocks), blocks nothing is cut from any more are pooled blocks again, and
// then a pooled block of the right size or a piece of a larger one (a slab) is taken; nullptr when the pool has nothing that large.  Until
// round 4's last session every such miss gave the WHOLE pool back (hipFree) and the following allocations came fresh from the driver, which
// clears what it hands out at ~25 GB/s: with the chunk indexes of a reference larger than the device built, mapped and dropped in turn
// (bench.py --config 5, 15 Gbp chunks) that happened once or twice per chunk — 5.6 s of a 7.0 s chunk build (MM_ALLOC_TRACE, tools/alloc_config5_small.sh).
inline void* big_pool_rescue(DevAlloc* self, int device, size_t bytes, size_t* got, bool caches_first) {
  // (the caches only for a device-filling build, which is after the whole blocks the mapping phase has cut its buffers from; given back at every refused
  // mid-size request they come straight back from the driver: config 4's 2.2 Gbp chunk builds beside 250 GB of pooled blocks went from 0.16 to 0.23 s)
  if (caches_first) { if (self) self->trim(); alloc_trim_others(self, device); }
  big_pool_adopt_idle(device);
  if (bytes >= alloc_env().index_scale) if (void* p = big_pool(device).take(bytes, got)) return p;
  if (bytes >= SLAB_FROM_BYTES) if (void* p = slab_piece(device, bytes)) { *got = SlabSet::granules(bytes); return p; }
  return nullptr;
}
// The ONE ladder of "the driver said out of memory: give memory back": the caller's own cache, the caches of the device's other contexts (the
// caches first: their pieces of pooled blocks go back to the blocks), the slabs that are idle by then, and then pooled blocks, largest first,
// until the driver can serve `need` bytes — or the whole pool (WHOLE_POOL; MM_NO_POOL_RESCUE=1; or when that did not make the room).
constexpr size_t WHOLE_POOL = (size_t)-1;
inline void reclaim(DevAlloc* self, int device, size_t need) {
  if (self) self->trim();
  alloc_trim_others(self, device);
  if (!(alloc_env().rescue && need != WHOLE_POOL && big_pool_trim_until(device, need))) big_pool_trim(device);
}
// ... and try again: reclaim, hipMalloc; still out of memory: the whole pool back, hipMalloc.  `refuse_below`: the request counts as refused, without
// asking the driver, while the device has less than this free behind the reclaim (DevAlloc::get's reserve for the runtime).
inline hipError_t retry_after_reclaim(void** p, size_t bytes, DevAlloc* self, int device, size_t need, size_t refuse_below = 0) {
  reclaim(self, device, need);
  size_t fr = 0, tot = 0;
  hipError_t e = hipErrorOutOfMemory;
  if (!(refuse_below && dev_mem_info(&fr, &tot) == hipSuccess && fr < refuse_below)) e = dev_malloc(p, bytes);
  if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); big_pool_trim(device); e = dev_malloc(p, bytes); }
  return e;
}
// A block straight from the driver, outside cache and pool; out of memory: every cache and the whole pool go first.
inline void* driver_block(size_t bytes, DevAlloc* self, int device) {
  void* p = nullptr;
  hipError_t e = dev_malloc(&p, bytes);
  if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); e = retry_after_reclaim(&p, bytes, self, device, WHOLE_POOL); }
  if (e != hipSuccess) throw_alloc_failed(bytes, e);
  return p;
}

// ---- a block for one context: from its cache, from a slab, from the driver
inline void* DevAlloc::get(size_t bytes, size_t* got) {
  const AllocEnv& E = alloc_env();
  const size_t want = round_up(bytes);
  if (void* p = take_cached(want, got)) return p;
  // The last GiB of the device stays with the runtime: a device filled to the brim by hipMalloc lets a later kernel launch fail inside the
  // runtime (its own allocations: HSA_STATUS_ERROR_OUT_OF_RESOURCES, the queue is aborted and the process with it — seen with three worker
  // contexts beside four resident chunk indexes); a request that would take it is treated as one that failed for lack of memory.
  const size_t RUNTIME_RESERVE = E.cap > 0 ? 0 : (size_t)1 << 30;   // (under the test hook MM_DEVICE_BYTES_CAP the "device" ends at the cap, far below the real one)
  bool roomy = false, refuse = false;
  if (want >= LARGE_FROM_BYTES) {                                // (headroom only while a fifth of the device is free: resident chunk indexes can leave less)
    size_t fr = 0, tot = 0;
    if (dev_mem_info(&fr, &tot) == hipSuccess) { roomy = device_roomy(fr, tot); refuse = fr < want + RUNTIME_RESERVE; }
  }
  // buffers of 256 KiB .. 64 MiB — per-read and per-candidate arrays — get the same quarter of headroom (no driver query: they cannot fill a device): without it every batch
  // with a few per cent more candidates than its worker context had seen went to the driver for ~50 blocks (round 6, tools/alloc_probe.sh: 141 driver allocations, 1.3 GB,
  // inside the bench's twelve timed steps)
  const size_t ask = ask_bytes(want, roomy);
  if (E.slabs && !eager && !in_build && want >= SLAB_FROM_BYTES) {
    const auto ts0 = TraceClock::now();
    if (void* q = slab_piece(device, ask)) { *got = SlabSet::granules(ask); alloc_trace("slab piece %zu bytes %.3f ms at %.1f ms\n", *got, ms_since(ts0), wall_ms()); return q; }
  }
  void* p = nullptr;
  const auto t0 = TraceClock::now();
  hipError_t e = refuse ? hipErrorOutOfMemory : dev_malloc(&p, ask);
  alloc_trace("hipMalloc %zu bytes %.3f ms at %.1f ms\n", ask, ms_since(t0), wall_ms());
  *got = ask;
  if (e == hipErrorOutOfMemory) {
    const int dv = dev_current();
    alloc_trace("out of memory at a request of %zu bytes (%zu bytes pooled)\n", want, big_pool_bytes(dv));
    (void)hipGetLastError();
    if (E.rescue && E.slabs) if (void* q = big_pool_rescue(this, dv, want, got, false)) { alloc_trace("... served from the pool (%zu bytes)\n", *got); return q; }
    *got = want;                                                 // (no headroom when memory is short)
    e = retry_after_reclaim(&p, want, this, dv, want + RUNTIME_RESERVE, refuse ? want + RUNTIME_RESERVE : 0);   // (refused, and still not there with every cache given back: refused again)
  }
  if (e != hipSuccess) throw_alloc_failed(want, e);
  return p;
}

// ---- an index-scale block: from the device's pool, else from the driver
inline void* index_scale_block(DevAlloc* owner, int device, size_t count_bytes, size_t* got) {
  // (the cache is only given up when the device is out of memory: trimming it before every index-scale allocation sent every
  // mid-size temporary of the next index build back to hipMalloc — 1 400 driver allocations per 25 builds, six of which stalled for
  // 6.1 s each on this runtime: MM_ALLOC_TRACE, round 3)
  const AllocEnv& E = alloc_env();
  const bool eager = owner && owner->eager;
  const auto t0 = TraceClock::now();
  BigPool& bp = big_pool(device);
  const size_t bytes = E.rescue ? index_scale_class(count_bytes) : count_bytes;   // (size classes: mm_alloc_rules.hpp)
  if (eager) owner->trim();                                      // (a device-filling build: nothing stays cached beside it ...)
  big_pool_adopt_idle(device);                                   // (blocks the mapping phase had cut its buffers from and has given back)
  void* p = bp.take(bytes, got);                                 // ... but a pooled block of the right size — the previous chunk index of a streaming pass — is taken:
                                                                 // a fresh block from the driver is cleared as it is handed out, 6 s of a 7 s build of a 15 Gbp chunk (round 4)
  if (!p && E.rescue && eager) {                                 // (device-filling builds only: the chunk builds of a --maxmemory run live on their context's cached blocks)
    // the mapping phase between two chunk builds cuts its buffers out of pooled blocks (slabs) and keeps them cached: with the caches given
    // back those blocks are whole again — the arrays of the previous chunk's index, which this build is about to ask for
    owner->trim(); alloc_trim_others(owner, device); big_pool_adopt_idle(device);
    p = bp.take(bytes, got);
    // (a piece of a LARGER pooled block before the driver is asked was tried too: the long-lived arrays then sit inside the blocks the next
    // arrays need whole, and the 62 GB occurrence array of a 15 Gbp chunk found neither a block nor room — out of memory with 33 GB free)
    if (p) alloc_trace("big block of %zu bytes for %zu after the caches went back\n", *got, bytes);
  }
  if (p) { alloc_trace("big block of %zu bytes reused for %zu\n", *got, bytes); return p; }
  *got = bytes;
  hipError_t e = dev_malloc(&p, bytes);
  if (e == hipErrorOutOfMemory) {
    alloc_trace("out of memory at an index-scale request of %zu bytes (%zu bytes pooled)\n", bytes, bp.bytes);
    (void)hipGetLastError();
    // before the ladder: a pooled block or a piece of one — for a device-filling build with the caches given back first, otherwise without and then with
    if (E.rescue) { p = big_pool_rescue(owner, device, bytes, got, eager); if (!p && !eager) p = big_pool_rescue(owner, device, bytes, got, true); }
    if (p) { e = hipSuccess; alloc_trace("... served from the pool (%zu bytes)\n", *got); }
    else { *got = bytes; e = retry_after_reclaim(&p, bytes, owner, device, bytes); }
  }
  if (e != hipSuccess) throw_alloc_failed(bytes, e);
  // (a rescued pooled block of exactly this size is reported here as well)
  if (E.trace && *got == bytes && !slab_set().owns(p)) alloc_trace("direct hipMalloc %zu bytes %.3f ms\n", bytes, ms_since(t0));
  return p;
}
// ... and back: index-scale blocks a build lets go of stay in the device's pool.
// Handing the sort buffers of a 26.8 Gbp build (~70 GB) back with hipFree made the FIRST allocations of the other contexts of the device wait
// 3.2 s in two runs of three (the worker contexts of `mapDirectly`: mapping phase 3.2 s instead of 0.23 s); pooled, 0 of 6.  What the pool holds
// is given up when an allocation fails for lack of memory (every allocation path trims it and tries again).
// `pooled_bytes` 0: a plain driver block of `plain_bytes` (driver_block), which goes back to the driver.
inline void release_uncached(void* p, size_t pooled_bytes, size_t plain_bytes, int device) {
  int cur = 0; (void)hipGetDevice(&cur);
  if (cur != device) (void)hipSetDevice(device);                 // the synchronisation below is for the block's device, whichever the calling thread is on
  (void)hipDeviceSynchronize();
  if (!pooled_bytes) dev_free(p, plain_bytes);
  else if (!slab_set().give_back(p, pooled_bytes)) big_pool(device).give(p, pooled_bytes);   // (nothing on the device still uses it: any context may take it; a piece of a larger pooled block returns to that block)
  if (cur != device) (void)hipSetDevice(cur);
}

template <typename T>
struct DBuf {
  T* p = nullptr;
  size_t n = 0;
  size_t block = 0;            // bytes of the underlying block (0 = index-scale block: big_bytes)
  size_t big_bytes = 0; int big_dev = 0;
  DevAlloc* owner = nullptr;
  // A block held jointly by several DBufs (share_from: the read-only minimizers and sketch hashes of a read batch, mapped against one
  // chunk index after the other): the block lives in `shared`, p / n alias it, the last holder's release frees it.
  std::shared_ptr<DBuf<T>> shared;
  DBuf() = default;
  explicit DBuf(size_t count) { alloc(count); }
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  DBuf(DBuf&& o) noexcept : p(o.p), n(o.n), block(o.block), big_bytes(o.big_bytes), big_dev(o.big_dev), owner(o.owner), shared(std::move(o.shared)) { o.p = nullptr; o.n = 0; }
  DBuf& operator=(DBuf&& o) noexcept {
    if (this != &o) { release(); p = o.p; n = o.n; block = o.block; big_bytes = o.big_bytes; big_dev = o.big_dev; owner = o.owner; shared = std::move(o.shared); o.p = nullptr; o.n = 0; }
    return *this;
  }
  ~DBuf() { release(); }
  void share_from(DBuf& src) {                                   // afterwards both hold the block; neither may write to it
    if (this == &src) return;
    release();
    if (!src.p) return;
    if (!src.shared) {
      auto sp = std::make_shared<DBuf<T>>();
      sp->p = src.p; sp->n = src.n; sp->block = src.block; sp->big_bytes = src.big_bytes; sp->big_dev = src.big_dev; sp->owner = src.owner;
      src.shared = std::move(sp);
    }
    shared = src.shared; p = shared->p; n = shared->n; block = 0; owner = nullptr;
  }
  void alloc(size_t count) {
    release();
    if (!count) return;
    const size_t bytes = count * sizeof(T);
    owner = current_alloc();
    block = 0; big_bytes = 0;
    if (bytes >= alloc_env().index_scale) { (void)hipGetDevice(&big_dev); p = (T*)index_scale_block(owner, big_dev, bytes, &big_bytes); }
    else if (owner) p = (T*)owner->get(bytes, &block);
    // no context bound to this thread: a plain driver block (not the index-scale pool, whose take() only matches requests within an eighth
    // of a block's size: small blocks would pile up there)
    else { (void)hipGetDevice(&big_dev); p = (T*)driver_block(bytes, nullptr, big_dev); }
    n = count;                                                   // (an allocation that failed has thrown: the buffer stays empty)
  }
  void release() {
    if (shared) { shared.reset(); p = nullptr; n = 0; block = 0; return; }
    if (p) {
      if (block && owner) owner->put(p, block);
      else release_uncached(p, big_bytes, n * sizeof(T), big_dev);
      p = nullptr;
    }
    n = 0; block = 0;
  }
  size_t bytes() const { return n * sizeof(T); }
  void zero(hipStream_t st) { if (n) MM_HIP(hipMemsetAsync(p, 0, bytes(), st)); }
  void upload(const T* h, size_t count, hipStream_t st) { if (count) MM_HIP(hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, st)); }
  void download(T* h, size_t count, hipStream_t st, size_t offset = 0) const {
    if (count) MM_HIP(hipMemcpyAsync(h, p + offset, count * sizeof(T), hipMemcpyDeviceToHost, st));
  }
  std::vector<T> to_host(hipStream_t st, size_t count = (size_t)-1) const {
    if (count == (size_t)-1) count = n;
    std::vector<T> v(count);
    download(v.data(), count, st);
    MM_HIP(mm::stream_sync(st));
    return v;
  }
};

// A device block outside cache and pool that only grows (K5's scratch, kept across batches).
struct GrowBuf {
  void* p = nullptr; size_t bytes = 0;
  void* at_least(DevAlloc& a, size_t want) {                     // (`a`: the context's allocator — its stream is waited for before the old block goes)
    if (want > bytes) {
      if (p) { MM_HIP(mm::stream_sync(a.stream)); release(); }
      p = driver_block(want, &a, a.device);
      bytes = want;
    }
    return p;
  }
  void release() { if (p) dev_free(p, bytes); p = nullptr; bytes = 0; }
};

}  // namespace mm
