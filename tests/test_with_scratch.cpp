// CPU harness: mm::with_scratch (metamaps_amd/csrc/mm_prims.hpp), the one statement of rocprim's two-call protocol, with a stub in place of
// the device buffer and fake calls in place of rocprim's: a call that reports 0 bytes, calls that report more and less than the buffer holds,
// calls that fail, and a buffer that stays empty.  Prints "ok <checks>" or the first fault.
#include <cstddef>
#include <cstdio>
#include <stdexcept>
#include <string>

// what the header takes from mm_common.hpp in the library's build
enum hipError_t { hipSuccess = 0, hipErrorUnknown = 999 };
enum { MM_ERR_DEVICE = 3 };
struct Thrown : std::runtime_error { int status; Thrown(int st, const std::string& m) : std::runtime_error(m), status(st) {} };
#define MM_HIP(expr) do { if ((expr) != hipSuccess) throw Thrown(MM_ERR_DEVICE, #expr); } while (0)
#define MM_REQUIRE(cond, st, msg) do { if (!(cond)) throw Thrown((st), (msg)); } while (0)
#include "../metamaps_amd/csrc/mm_prims.hpp"

struct Buf {                                                      // DBuf<uint8_t>'s p, n and alloc; `broken`: alloc leaves it empty
  unsigned char* p = nullptr; size_t n = 0; int allocs = 0; bool broken = false;
  unsigned char block[4096];
  void alloc(size_t count) { ++allocs; p = nullptr; n = 0; if (!count || broken || count > sizeof block) return; p = block; n = count; }
};
struct Fake {                                                     // reports `want` bytes to a null pointer, "runs" with any other
  size_t want; hipError_t query_err = hipSuccess, run_err = hipSuccess;
  int queries = 0, runs = 0; void* ran_with = nullptr; size_t ran_bytes = (size_t)-1;
  hipError_t operator()(void* tmp, size_t& bytes) {
    if (!tmp) { ++queries; bytes = want; return query_err; }
    ++runs; ran_with = tmp; ran_bytes = bytes; return run_err;
  }
};

static int checks = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

// one call on `b`: the query and the run happen once each, the run gets the buffer and the reported size, the buffer holds max(want, 16)
static int one_call(Buf& b, size_t want) {
  const size_t before = b.n;
  Fake f{want};
  mm::with_scratch(b, f);
  CHECK(f.queries == 1 && f.runs == 1);
  CHECK(b.p != nullptr && f.ran_with == (void*)b.p && f.ran_bytes == want);
  CHECK(b.n >= (want > 16 ? want : 16));
  CHECK(b.n >= before);                                           // never shrunk
  return 0;
}

int main() {
  Buf b;
  if (one_call(b, 0)) return 1;                                   // an empty buffer and a call that wants nothing: still a buffer
  CHECK(b.allocs == 1 && b.n == 16);
  if (one_call(b, 0)) return 1;
  if (one_call(b, 16)) return 1;
  CHECK(b.allocs == 1);                                           // (what it holds is enough)
  if (one_call(b, 1000)) return 1;                                // more than it holds: grown
  CHECK(b.allocs == 2 && b.n == 1000);
  if (one_call(b, 100)) return 1;                                 // less: kept as it is
  if (one_call(b, 0)) return 1;
  if (one_call(b, 1000)) return 1;
  CHECK(b.allocs == 2 && b.n == 1000);
  if (one_call(b, 1001)) return 1;
  CHECK(b.allocs == 3);
  CHECK(mm::scratch_bytes(Fake{77}) == 77);                       // the query alone

  { Fake f{64}; f.query_err = hipErrorUnknown; bool threw = false;   // a failed query: no run
    try { mm::with_scratch(b, f); } catch (const Thrown&) { threw = true; }
    CHECK(threw && f.queries == 1 && f.runs == 0); }
  { Fake f{64}; f.run_err = hipErrorUnknown; bool threw = false;     // a failed run is reported
    try { mm::with_scratch(b, f); } catch (const Thrown&) { threw = true; }
    CHECK(threw && f.queries == 1 && f.runs == 1); }
  { Buf e; e.broken = true; Fake f{0}; bool threw = false;           // a buffer that stays empty: refused before the run, which would be a second query
    try { mm::with_scratch(e, f); } catch (const Thrown& t) { threw = t.status == MM_ERR_DEVICE; }
    CHECK(threw && f.queries == 1 && f.runs == 0 && e.p == nullptr); }
  printf("ok %d\n", checks);
  return 0;
}
