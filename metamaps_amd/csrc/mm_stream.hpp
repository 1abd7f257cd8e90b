// Waiting for a stream (host side).  Every wait of the library goes through stream_sync.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include "cpu_budget.hpp"

namespace mm {

// ---- waiting for a stream ------------------------------------------------------------------------------
// hipStreamSynchronize spins: a host thread per context burns a CPU while its kernels run.  On a host with CPUs to spare that is the lowest
// latency; in a container with a small CPU quota (cpu_budget.hpp) four spinning workers are a quarter of the quota gone, and once the quota of
// a 100 ms period is used up the kernel stops every thread of the process.  So when the budget is small (<= 32 CPUs) a wait records an event
// created with hipEventBlockingSync and sleeps on it instead (an interrupt wakes the thread; 10-30 us later than a spin would have noticed).
// MM_SYNC=spin|block overrides.  Every wait of the library goes through here.
inline bool sync_blocking() {
  static const bool b = [] { const char* e = getenv("MM_SYNC"); if (e && *e) return strcmp(e, "block") == 0; return cpu_budget() <= 32; }();
  return b;
}
// The event a wait sleeps on belongs to the stream: a context registers one with its stream when it is created (mm_ctx_create, aux_ready) and takes
// it back when it goes (mm_ctx_destroy) — no event per host thread (the CLI's worker, pool and on_each threads are created per run and never destroyed
// theirs), no hipGetDevice per wait, and a thread whose current device is another one (the allocator trimming a foreign context's cache) sleeps too
// instead of falling back to the spin.  Streams nobody registered (none in the product) keep the thread-local event.
// A stream's event is shared by every thread that waits for the stream — its context's own thread, and any thread that trims the context's cache
// when the device is full (reclaim, mm_alloc.hpp) — so an entry carries a mutex that is held across record and wait, and under which the event is
// destroyed: two threads never record or wait on one event at once, and a waiter that found the entry before it was unregistered finds it empty.
struct StreamEvents {
  struct Entry { std::mutex mu; hipEvent_t ev = nullptr; };
  std::mutex mu;
  std::map<hipStream_t, std::shared_ptr<Entry>> ev;
  static StreamEvents& get() { static StreamEvents* s = new StreamEvents; return *s; }   // (never destroyed: contexts may outlive static destruction)
  static std::shared_ptr<Entry> find(hipStream_t st) {
    StreamEvents& S = get();
    std::lock_guard<std::mutex> g(S.mu);
    auto it = S.ev.find(st);
    return it == S.ev.end() ? nullptr : it->second;
  }
};
inline void stream_event_register(hipStream_t st) {                // (the stream's device is current)
  if (!sync_blocking()) return;
  auto en = std::make_shared<StreamEvents::Entry>();
  if (hipEventCreateWithFlags(&en->ev, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return; }
  StreamEvents& S = StreamEvents::get();
  std::lock_guard<std::mutex> g(S.mu);
  S.ev[st] = std::move(en);
}
inline void stream_event_unregister(hipStream_t st) {
  StreamEvents& S = StreamEvents::get();
  std::shared_ptr<StreamEvents::Entry> en;
  { std::lock_guard<std::mutex> g(S.mu); auto it = S.ev.find(st); if (it != S.ev.end()) { en = std::move(it->second); S.ev.erase(it); } }
  if (!en) return;
  std::lock_guard<std::mutex> g(en->mu);                          // (a wait in flight ends first)
  if (en->ev) (void)hipEventDestroy(en->ev);
  en->ev = nullptr;
}
inline hipError_t event_wait(hipEvent_t ev, hipStream_t st) {      // (the caller is the only user of `ev` for the duration)
  if (hipEventRecord(ev, st) != hipSuccess) { (void)hipGetLastError(); return hipStreamSynchronize(st); }
  const hipError_t w = hipEventSynchronize(ev);
  if (w != hipSuccess) { (void)hipGetLastError(); return hipStreamSynchronize(st); }
  return hipSuccess;
}
inline hipEvent_t thread_event() {                                 // a stream without a registered event: one event per thread and device; nullptr: none to be had
  static thread_local hipEvent_t tev = nullptr; static thread_local int ev_dev = -1;
  int dev = 0; (void)hipGetDevice(&dev);
  if (!tev || ev_dev != dev) {
    if (tev) (void)hipEventDestroy(tev);
    tev = nullptr;
    if (hipEventCreateWithFlags(&tev, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess) { tev = nullptr; (void)hipGetLastError(); return nullptr; }
    ev_dev = dev;
  }
  return tev;
}
inline hipError_t stream_sync(hipStream_t st) {
  if (!sync_blocking()) return hipStreamSynchronize(st);
  if (auto en = StreamEvents::find(st)) {
    std::lock_guard<std::mutex> g(en->mu);
    if (en->ev) return event_wait(en->ev, st);
  }
  const hipEvent_t tev = thread_event();
  return tev ? event_wait(tev, st) : hipStreamSynchronize(st);
}

}  // namespace mm
