// The sizing rules of the device allocator (mm_alloc.hpp): pure arithmetic, no HIP call in here — tests/test_alloc_rules.cpp holds them against
// their formulas on the CPU.  The measured reasons for each rule stand where it is used.
#pragma once
#include <algorithm>
#include <cstddef>

namespace mm {

constexpr size_t SLAB_FROM_BYTES = (size_t)1 << 20;             // smaller requests stay with the driver (they come from its own small pools, quickly)
constexpr size_t MID_FROM_BYTES = (size_t)256 << 10;            // from here on a cached block may be 60 % too large, and a driver block gets headroom
constexpr size_t LARGE_FROM_BYTES = (size_t)64 << 20;           // from here on headroom depends on how full the device is (the driver is asked)

// what a cached block is asked for as: 4 KiB at least, then an eighth of the size's power of two
inline size_t round_up(size_t b) {
  if (b < 4096) return 4096;
  int lg = 63 - __builtin_clzll((unsigned long long)b);
  size_t gran = (size_t)1 << (lg > 3 ? lg - 3 : 0);             // <= 12.5 % slack
  return (b + gran - 1) / gran * gran;
}
// a cached block of `have` bytes serves a (rounded) request of `want`: at most a quarter too large, 60 % from 256 KiB on
inline bool cache_fits(size_t have, size_t want) {
  return have >= want && have <= want + want / 4 + (want >= MID_FROM_BYTES ? want * 7 / 20 : 0);
}
// what the driver is asked for to serve a (rounded) request of `want`: a quarter more from 256 KiB on, from 64 MiB on only while
// `roomy` (a fifth of the device is free)
inline size_t ask_bytes(size_t want, bool roomy) {
  if (want >= LARGE_FROM_BYTES ? roomy : want >= MID_FROM_BYTES) return round_up(want + want / 4);
  return want;
}
inline bool device_roomy(size_t free_bytes, size_t total_bytes) { return free_bytes > total_bytes / 5; }
// Index-scale blocks come in size classes (a 64th of the size's power of two, at least 16 MiB: <= 1.6 % slack): the chunk indexes of a
// pass differ by a fraction of a percent, and a pooled block a few KB too small for the next chunk's array is a miss
inline size_t index_scale_class(size_t b) {
  int lg = 63 - __builtin_clzll((unsigned long long)std::max<size_t>(b, 1));
  const size_t gran = std::max<size_t>((size_t)1 << (lg > 6 ? lg - 6 : 0), (size_t)16 << 20);
  return (b + gran - 1) / gran * gran;
}
// a pooled index-scale block of `have` bytes serves a request of `want`: at most an eighth too large (index-scale blocks are what fills the device)
inline bool pool_block_fits(size_t have, size_t want) { return have >= want && have <= want + want / 8; }

}  // namespace mm
