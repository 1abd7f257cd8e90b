// The device primitives that the library's sort, scan and per-read code share (included by the .hip files only).
//   host    with_scratch: the two-call protocol of rocprim, once; sort_keys / sort_pairs / exclusive_scan / inclusive_scan_max on top of it; bits_for, flat_grid,
//           fill_iota, rank_by_bits; StageClock, the event-pair clock behind MM_GENE_TIMING and MM_IDENT_TIMING
//   device  Lanes<W>, the butterflies of W consecutive lanes; for_each_read_tile, the loop of the per-read kernels (mm_lca.hip, mm_ident.hip)
// with_scratch alone compiles without the HIP runtime (tests/test_with_scratch.cpp via g++, with a stub in place of DBuf).
#pragma once
#include <algorithm>
#include <cstdint>
#ifdef __HIPCC__
#include "mm_common.hpp"
#include <rocprim/rocprim.hpp>
#endif

namespace mm {

// rocprim's calls take (scratch pointer, scratch bytes, ...) and read a NULL pointer as "tell me the bytes".  `call` is one of them as
// hipError_t(void* tmp, size_t& bytes).  A buffer of 0 bytes would be a null pointer: the second call would be another query and the work
// would silently not run.  So the buffer holds at least 16 bytes, and its pointer is checked.  `tmp` (DBuf<uint8_t>, or the test's stub)
// grows and never shrinks: a job passes the same one to all of its calls.
template <class Call> size_t scratch_bytes(Call&& call) { size_t bytes = 0; MM_HIP(call(nullptr, bytes)); return bytes; }   // (the query alone)
template <class Buf, class Call> void with_scratch(Buf& tmp, Call&& call) {
  size_t bytes = scratch_bytes(call);
  const size_t want = std::max<size_t>(bytes, 16);
  if (tmp.n < want) tmp.alloc(want);
  MM_REQUIRE(tmp.p != nullptr, MM_ERR_DEVICE, "a device primitive got no scratch buffer: it would report a size and not run");
  MM_HIP(call((void*)tmp.p, bytes));
}

#ifdef __HIPCC__
template <class Call> void with_scratch(Call&& call) { DBuf<uint8_t> tmp; with_scratch(tmp, call); }   // (a buffer of this call alone)

// the bits [bit0, bit1) of the keys decide the order; stable
template <class K> void sort_keys(DBuf<uint8_t>& tmp, K* src, K* dst, size_t n, int bit0, int bit1, hipStream_t st) {
  with_scratch(tmp, [&](void* t, size_t& b) { return rocprim::radix_sort_keys(t, b, src, dst, n, (unsigned)bit0, (unsigned)bit1, st); });
}
template <class K, class V> void sort_pairs(DBuf<uint8_t>& tmp, K* kin, K* kout, V* vin, V* vout, size_t n, int bit0, int bit1, hipStream_t st) {
  with_scratch(tmp, [&](void* t, size_t& b) { return rocprim::radix_sort_pairs(t, b, kin, kout, vin, vout, n, (unsigned)bit0, (unsigned)bit1, st); });
}
template <class In, class Out> void exclusive_scan(DBuf<uint8_t>& tmp, const In* src, Out* dst, size_t n, hipStream_t st) {   // sums in Out, from 0
  with_scratch(tmp, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, src, dst, (Out)0, n, rocprim::plus<Out>(), st); });
}
template <class T> void inclusive_scan_max(DBuf<uint8_t>& tmp, const T* src, T* dst, size_t n, hipStream_t st) {   // dst[i]: the largest of src[0 .. i]
  with_scratch(tmp, [&](void* t, size_t& b) { return rocprim::inclusive_scan(t, b, src, dst, n, rocprim::maximum<T>(), st); });
}

inline int bits_for(uint64_t n) { int b = 1; while (b < 64 && (n >> b)) ++b; return b; }   // bits that hold 0 .. n
inline unsigned flat_grid(int64_t n) { return (unsigned)std::max<int64_t>(ceil_div(n, 256), 1); }   // workgroups of 256 threads, one per element

// (iota and the ranking are templates so that only the files that use them get their kernels, rocprim's sort among them)
template <class T> __global__ void __launch_bounds__(256) iota_kernel(T* __restrict__ v, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) v[i] = (T)i;
}
template <class T> void fill_iota(T* v, int64_t n, hipStream_t st) { iota_kernel<<<dim3(flat_grid(n)), dim3(256), 0, st>>>(v, n); MM_KERNEL_CHECK(); }
// the order of n 64-bit patterns (non-negative doubles order as theirs): sorted[i] ascending, perm[i] the index in `bits` of sorted[i];
// equal patterns keep their order.  iota: n words of the caller's.
template <class I> void rank_by_bits(DBuf<uint8_t>& tmp, uint64_t* bits, uint64_t* sorted, I* iota, I* perm, size_t n, hipStream_t st) {
  fill_iota(iota, (int64_t)n, st);
  sort_pairs(tmp, bits, sorted, iota, perm, n, 0, 64, st);
}

// The device times of a job's N stages, one pair of events on its stream: start(), the stage's launches, stop(k) (which waits for them).
// Off, it records nothing.  The job prints ms[] in its own format.
template <int N> struct StageClock {
  const bool on; hipStream_t st; hipEvent_t a = nullptr, b = nullptr;
  double ms[N] = {};
  StageClock(bool on_, hipStream_t s) : on(on_), st(s) { if (on) { MM_HIP(hipEventCreate(&a)); MM_HIP(hipEventCreate(&b)); } }
  ~StageClock() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  void start() { if (on) MM_HIP(hipEventRecord(a, st)); }
  void stop(int k) { if (!on) return; MM_HIP(hipEventRecord(b, st)); MM_HIP(hipEventSynchronize(b)); float t = 0; MM_HIP(hipEventElapsedTime(&t, a, b)); ms[k] += t; }
};

// ---- device -------------------------------------------------------------------------------------------------------------------------------
template <int W> struct Lanes {                                   // W consecutive lanes of a wavefront (W a power of two)
  __device__ int lane() const { return (int)(threadIdx.x & (W - 1)); }
  __device__ int width() const { return W; }
  __device__ double sum(double x) const { for (int d = W / 2; d > 0; d >>= 1) x += __shfl_xor(x, d, W); return x; }   // (butterflies: the same bits in every lane)
  __device__ int32_t min(int32_t x) const { for (int d = W / 2; d > 0; d >>= 1) x = ::min(x, __shfl_xor(x, d, W)); return x; }
  __device__ int32_t max(int32_t x) const { for (int d = W / 2; d > 0; d >>= 1) x = ::max(x, __shfl_xor(x, d, W)); return x; }
  __device__ uint64_t max(uint64_t x) const {
    for (int d = W / 2; d > 0; d >>= 1) { const uint64_t y = (uint64_t)__shfl_xor((unsigned long long)x, d, W); x = y > x ? y : x; }
    return x;
  }
  __device__ bool any(bool b) const { return __any(b) != 0; }     // of the whole wavefront
};

// The reads [0, n_reads) with entries [read_off[r], read_off[r + 1]), for kernels of 256 threads on a grid of read_tile_grid<GROUP>: a
// wavefront takes tiles of 64 / GROUP consecutive reads.
//   short_fn(r, lo, n, mine, gl)  once per tile, by all 64 lanes: the group of GROUP lanes that this lane (gl of its group) belongs to has
//                                 read r, which is its own to handle (mine) if it exists and has n <= GROUP entries, none included; a read
//                                 beyond the last arrives as lo = n = 0
//   long_fn(r, lo, n)             once per read of the tile with n > GROUP, by all 64 lanes
// The bounds of both loops are the same for every lane of a wavefront, so each of them reaches every shuffle of the two functions.
template <int GROUP, class ShortFn, class LongFn>
__device__ __forceinline__ void for_each_read_tile(const int64_t* read_off, int64_t n_reads, ShortFn&& short_fn, LongFn&& long_fn) {
  constexpr int PER_WAVE = 64 / GROUP;
  const int lane = threadIdx.x & 63, gl = lane & (GROUP - 1), grp = lane / GROUP;
  const int64_t n_waves = (int64_t)gridDim.x * 4, wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  for (int64_t r0 = wave * PER_WAVE; r0 < n_reads; r0 += n_waves * PER_WAVE) {
    const int64_t r = r0 + grp;
    int64_t lo = 0, n = 0;
    if (r < n_reads) { lo = read_off[r]; n = read_off[r + 1] - lo; }
    short_fn(r, lo, n, r < n_reads && n <= GROUP, gl);
    for (int q = 0; q < PER_WAVE && r0 + q < n_reads; ++q) {
      const int64_t qlo = read_off[r0 + q], qn = read_off[r0 + q + 1] - qlo;
      if (qn > GROUP) long_fn(r0 + q, qlo, qn);
    }
  }
}
template <int GROUP> unsigned read_tile_grid(int64_t n_reads) { return (unsigned)std::min<int64_t>(ceil_div(n_reads, 256 / GROUP), 2048); }
#endif

}  // namespace mm
