// The device's lane policy of the inflate cores (mm_inflate.hpp, mm_gzip.hpp): one wavefront, its bit reader fed from an LDS ring of the
// compressed bytes.  Shared by the BGZF kernel (mm_inflate.hip) and the plain gzip kernels (mm_gzip.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mmi {

constexpr uint32_t RING = 4096, RING_CHUNK = 2048;              // the input ring in LDS and what one cooperative load adds to it

struct WaveLanes {
  static constexpr uint32_t W = 64;
  uint8_t* ring;                                                 // input bytes [loaded - RING, loaded) at ring[pos % RING]
  const uint8_t* gin = nullptr; uint32_t glen = 0, loaded = 0;
  __device__ uint32_t lane() const { return threadIdx.x; }
  __device__ uint64_t ballot(bool b) const { return __ballot(b); }
  __device__ uint32_t popc(uint64_t m) const { return (uint32_t)__popcll(m); }
  __device__ uint32_t popc_below(uint64_t m) const { return (uint32_t)__popcll(m & ((1ull << threadIdx.x) - 1)); }
  __device__ void sync() const { __syncthreads(); }
  __device__ uint32_t xor_all(uint32_t v) const {
#pragma unroll
    for (int o = 32; o; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
  }
  // The bit reader reads the block's deflate bytes from an LDS ring the wave fills 2 KiB at a time with coalesced loads: a global load per
  // refill made every symbol wait out a memory latency.  ensure() runs in wave-uniform control flow (every Bits::fill).  pos only grows, and
  // a load never goes past pos + 64 + RING_CHUNK, so the bytes the reader still needs are not overwritten.
  __device__ void begin_input(const uint8_t* in, uint32_t n) { gin = in; glen = n; loaded = 0; }
  __device__ void ensure(uint32_t pos) {
    if (loaded >= pos + 64 || loaded >= glen) return;
    if (loaded < pos) loaded = pos;                              // (a stored block skipped ahead)
    __syncthreads();                                             // (every lane is done with the bytes the load replaces)
    while (loaded < pos + 64 && loaded < glen) {
      const uint32_t m = glen - loaded < RING_CHUNK ? glen - loaded : RING_CHUNK;
      for (uint32_t i = threadIdx.x; i < m; i += 64) ring[(loaded + i) % RING] = gin[loaded + i];
      loaded += m;
    }
    __syncthreads();
  }
  __device__ uint8_t in_byte(const uint8_t*, uint32_t n, uint32_t pos) const { return pos < n ? ring[pos % RING] : 0; }
};

}  // namespace mmi
