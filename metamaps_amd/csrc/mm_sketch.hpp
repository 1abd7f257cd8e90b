// K2 kernels — the sketch of a read = its minimizers sorted by hash, unique (computeMap.hpp:292-298) — and the copy kernels of the
// duplicate-hash strand tie-break.  Included by mm_map.hip alone.
#pragma once
#include <rocprim/rocprim.hpp>
#include "mm_map.hpp"

namespace mm {

// ---------------------------------------------------------------------------------------------------
// K2  sketch: one workgroup per read
// ---------------------------------------------------------------------------------------------------
// Up to 16 384 minimizers: an LDS radix sort by hash (stable, so equal hashes stay in winnowing order), then unique + strand.
// IPT = elements per thread; 256 * IPT >= minimizers of the longest read of the class.
template <int IPT>
__global__ void __launch_bounds__(256) sketch_radix_kernel(const Rec* __restrict__ rec, const uint64_t* __restrict__ off,
                                                           const int32_t* __restrict__ read_list, uint32_t* __restrict__ sk_hash,
                                                           uint8_t* __restrict__ sk_strand, int32_t* __restrict__ sk_n, uint8_t* __restrict__ amb) {
  using Sort = rocprim::block_radix_sort<uint32_t, 256, IPT, uint16_t>;
  using Scan = rocprim::block_scan<int, 256>;
  union Tmp { typename Sort::storage_type sort; typename Scan::storage_type scan; };
  extern __shared__ __align__(16) unsigned char sketch_dyn[];    // dynamic: 64 elements per thread need more than 64 KB
  Tmp& tmp = *reinterpret_cast<Tmp*>(sketch_dyn);
  __shared__ uint32_t last_key[256];
  __shared__ uint8_t last_st[256];
  __shared__ int s_amb;
  const int r = read_list[blockIdx.x];
  const uint64_t o = off[r];
  const int n = (int)(off[r + 1] - o);
  const int t = threadIdx.x;
  uint32_t key[IPT]; uint16_t val[IPT];
#pragma unroll
  for (int i = 0; i < IPT; ++i) { const int idx = t * IPT + i; key[i] = idx < n ? rec[o + idx].hash : 0xffffffffu; val[i] = (uint16_t)idx; }
  if (t == 0) s_amb = 0;
  Sort().sort(key, val, tmp.sort);                               // blocked: thread t holds sorted positions t*IPT ..
  uint8_t stv[IPT];
#pragma unroll
  for (int i = 0; i < IPT; ++i) stv[i] = (t * IPT + i < n) ? (uint8_t)(rec[o + val[i]].pw & PW_STRAND) : 0;
  last_key[t] = key[IPT - 1]; last_st[t] = stv[IPT - 1];
  __syncthreads();
  int nfirst = 0; bool first[IPT]; bool ambig = false;
#pragma unroll
  for (int i = 0; i < IPT; ++i) {
    const int pos = t * IPT + i;
    const uint32_t pk = i ? key[i - 1] : (t ? last_key[t - 1] : 0u);
    const uint8_t ps = i ? stv[i - 1] : (t ? last_st[t - 1] : 0);
    first[i] = pos < n && (pos == 0 || pk != key[i]);
    if (pos < n && pos > 0 && pk == key[i] && ps != stv[i]) ambig = true;   // same hash, different strands
    nfirst += first[i] ? 1 : 0;
  }
  if (ambig) s_amb = 1;
  int ex = 0, total = 0;
  Scan().exclusive_scan(nfirst, ex, 0, total, tmp.scan);
  const int ex0 = ex;
#pragma unroll
  for (int i = 0; i < IPT; ++i) if (first[i]) { sk_hash[o + ex] = key[i]; sk_strand[o + ex] = stv[i]; ++ex; }
  __threadfence_block();
  __syncthreads();
  // bit 1 of the strand byte: some duplicate of this hash has the other strand, i.e. the strand the reference would keep
  // depends on libstdc++'s sort (resolved on the host, and only if a strand vote ever reads this entry)
  if (s_amb) {
    int ex2 = ex0;
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
      const int pos = t * IPT + i;
      if (first[i]) ++ex2;
      const uint32_t pk = i ? key[i - 1] : (t ? last_key[t - 1] : 0u);
      const uint8_t ps = i ? stv[i - 1] : (t ? last_st[t - 1] : 0);
      if (pos < n && pos > 0 && pk == key[i] && ps != stv[i]) sk_strand[o + ex2 - 1] |= 2;
    }
  }
  if (t == 0) { sk_n[r] = total; amb[r] = (uint8_t)(s_amb ? 2 : 0); }   // 2: ambiguous entries are marked
}

// Sketches of more than 16 384 minimizers (reads beyond ~73 kb): (hash << 32 | winnowing index) keys of the listed reads back to back
// in one buffer, one segmented device radix sort, then unique + strand per read from the sorted keys, with sketch_radix_kernel's
// per-entry ambiguity marks, so that these reads take the lazy strand tie-break too.
__global__ void __launch_bounds__(256) sketch_keys_kernel(const Rec* __restrict__ rec, const uint64_t* __restrict__ off, const int32_t* __restrict__ read_list,
                                                          const uint64_t* __restrict__ koff, uint64_t* __restrict__ keys) {
  const int r = read_list[blockIdx.x];
  const uint64_t o = off[r], k0 = koff[blockIdx.x];
  const uint32_t n = (uint32_t)(off[r + 1] - o);
  for (uint32_t i = threadIdx.x; i < n; i += 256) keys[k0 + i] = ((uint64_t)rec[o + i].hash << 32) | i;
}
__global__ void __launch_bounds__(256) sketch_finish_kernel(const Rec* __restrict__ rec, const uint64_t* __restrict__ off, const int32_t* __restrict__ read_list,
                                                            const uint64_t* __restrict__ koff, const uint64_t* __restrict__ sorted,
                                                            uint32_t* __restrict__ sk_hash, uint8_t* __restrict__ sk_strand, int32_t* __restrict__ sk_n, uint8_t* __restrict__ amb) {
  const int r = read_list[blockIdx.x];
  const uint64_t o = off[r];
  const uint64_t* __restrict__ a = sorted + koff[blockIdx.x];
  const int n = (int)(off[r + 1] - o);
  __shared__ int s_amb;
  if (threadIdx.x == 0) s_amb = 0;
  __syncthreads();
  for (int pass = 0; pass < 2; ++pass) {                          // 0: survivors (first of every run of equal hashes); 1: marks on them
    uint64_t carry = 0;
    for (int base = 0; base < n; base += 256) {
      const int i = base + threadIdx.x;
      bool first = false, differs = false; uint32_t h = 0, stv = 0;
      if (i < n) {
        const uint64_t key = a[i];
        h = (uint32_t)(key >> 32);
        stv = rec[o + (uint32_t)key].pw & PW_STRAND;
        if (i == 0) first = true;
        else {
          const uint64_t pk = a[i - 1];
          first = (uint32_t)(pk >> 32) != h;
          differs = !first && (rec[o + (uint32_t)pk].pw & PW_STRAND) != stv;   // same hash, different strands
        }
      }
      uint64_t tot;
      const uint64_t ex = block_excl_scan_u64(first ? 1 : 0, &tot);
      if (pass == 0) {
        if (first) { sk_hash[o + carry + ex] = h; sk_strand[o + carry + ex] = (uint8_t)stv; }
        if (differs) s_amb = 1;
      } else if (differs) sk_strand[o + carry + ex - 1] |= 2;     // bit 1 on the run's survivor (the last first at or before i): strand unresolved
      carry += tot;
    }
    __threadfence_block();
    __syncthreads();
    if (pass == 0) {
      if (threadIdx.x == 0) { sk_n[r] = (int32_t)carry; amb[r] = (uint8_t)(s_amb ? 2 : 0); }   // 2: ambiguous entries are marked (lazy tie-break)
      if (!s_amb) break;
    }
  }
}

// compact copies for the host-side duplicate-hash tie-break (one workgroup per flagged read)
__global__ void __launch_bounds__(256) gather_amb_kernel(const Rec* __restrict__ rec, const uint64_t* __restrict__ src_off,
                                                         const uint64_t* __restrict__ dst_off, Rec* __restrict__ out) {
  const uint64_t so = src_off[blockIdx.x], d0 = dst_off[blockIdx.x], n = dst_off[blockIdx.x + 1] - d0;
  for (uint64_t i = threadIdx.x; i < n; i += 256) out[d0 + i] = rec[so + i];
}
__global__ void __launch_bounds__(256) scatter_strand_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ src_off,
                                                             const uint64_t* __restrict__ dst_off, const int32_t* __restrict__ cnt,
                                                             uint8_t* __restrict__ sk_strand) {
  const uint64_t d0 = dst_off[blockIdx.x], so = src_off[blockIdx.x];
  const int n = cnt[blockIdx.x];
  for (int i = threadIdx.x; i < n; i += 256) sk_strand[so + i] = in[d0 + i];
}

}  // namespace mm
