// K4 kernels — hit sort and L1 candidate scan (computeMap.hpp:346-386) — the K5 grouping / range kernels and the record compaction.
// Included by mm_map.hip alone, behind mm_l2.hpp.
#pragma once
#include <rocprim/rocprim.hpp>
#include "mm_map.hpp"
#include "mm_l2.hpp"

namespace mm {

// ---------------------------------------------------------------------------------------------------
// K4a  sort the seed hits of each read by (contig, wpos)          computeMap.hpp:353
// ---------------------------------------------------------------------------------------------------
// Up to 4096 hits: an LDS radix sort over the significant key bits (contig in the high word, position and strand below it).
// 256 * IPT >= hits of the longest read of the class.  Longer lists take the device's segmented radix sort (MapRun::sort_hits_segmented).
template <int IPT>
__global__ void __launch_bounds__(256) sort_hits_radix_kernel(uint64_t* __restrict__ hits, const uint64_t* __restrict__ read_hit_off,
                                                              const int32_t* __restrict__ read_list, int end_bit,
                                                              const uint64_t* __restrict__ stage /* optional: staged survivors of the filter ... */,
                                                              const uint64_t* __restrict__ stage_off /* ... which hold a read's hits whenever they fit its stage */) {
  using Sort = rocprim::block_radix_sort<uint64_t, 256, IPT>;
  extern __shared__ __align__(16) unsigned char sort_dyn[];
  typename Sort::storage_type& tmp = *reinterpret_cast<typename Sort::storage_type*>(sort_dyn);
  const int r = read_list[blockIdx.x];
  const uint64_t o = read_hit_off[r];
  const int n = (int)(read_hit_off[r + 1] - o);
  const uint64_t* __restrict__ src = hits + o;
  if (stage) { const uint64_t sb = stage_off[r]; if ((uint64_t)n <= stage_off[r + 1] - sb) src = stage + sb; }   // (then the filter's write kernel left hits[] alone)
  uint64_t key[IPT];
#pragma unroll
  for (int i = 0; i < IPT; ++i) { const int idx = threadIdx.x * IPT + i; key[i] = idx < n ? src[idx] : ~0ull; }
  Sort().sort(key, tmp, 0, end_bit);                             // blocked: thread t holds sorted positions t*IPT ..  (padding keys sort last)
#pragma unroll
  for (int i = 0; i < IPT; ++i) { const int idx = threadIdx.x * IPT + i; if (idx < n) hits[o + idx] = key[i]; }
}

// ---------------------------------------------------------------------------------------------------
// K4b  L1 candidate scan, one thread per read, the reference's loop verbatim in behaviour
//      (computeL1CandidateRegions, computeMap.hpp:346-386).  WRITE=false counts, WRITE=true writes.
// ---------------------------------------------------------------------------------------------------
template <bool WRITE>
__global__ void l1_scan_kernel(const uint64_t* __restrict__ hits, const uint64_t* __restrict__ read_hit_off, const int32_t* __restrict__ read_len,
                               const int32_t* __restrict__ min_hits, int64_t n_reads, uint32_t* __restrict__ cand_n,
                               const uint64_t* __restrict__ cand_off, int32_t* __restrict__ cand, int32_t* __restrict__ cand_read) {
  int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_reads) return;
  const uint64_t o = read_hit_off[r];
  const int64_t H = (int64_t)(read_hit_off[r + 1] - o);
  const int len = read_len[r];
  int m = min_hits[r]; if (m < 1) m = 1;                         // :349
  uint32_t nc = 0;
  int lseq = -1, lstart = 0, lend = 0;
  uint64_t wbase = WRITE ? cand_off[r] : 0;
  auto flush = [&]() {
    if (lseq < 0) return;
    if (WRITE) { int32_t* c = cand + 3 * (wbase + nc); c[0] = lseq; c[1] = lstart; c[2] = lend; cand_read[wbase + nc] = (int32_t)r; }
    ++nc;
  };
  for (int64_t i = 0; i + m <= H; ++i) {
    uint64_t a = hits[o + i], b = hits[o + i + m - 1];
    int sa = (int)(a >> 32), sb = (int)(b >> 32);
    int wa = pw_wpos((uint32_t)a), wb = pw_wpos((uint32_t)b);
    if (sa != sb || wb - wa >= len) continue;                    // :365
    int cs = max(0, wb - len + 1), ce = wa;                      // :368
    if (lseq == sa && lend >= cs) lend = max(ce, lend);          // :374-380
    else { flush(); lseq = sa; lstart = cs; lend = ce; }
  }
  flush();
  if (!WRITE) cand_n[r] = nc;
}

// The same loop, one wavefront per read.  Hits are sorted by (contig, position), so the merged region so far ends at the
// position of the latest qualifying hit: hit i opens a new candidate iff the previous qualifying hit lies on another contig
// or before max(0, wpos[i+m-1]-len+1).  That makes every decision local (ballot + one shuffle); a candidate's end is written
// by the last qualifying hit before the next opening one, later chunks of the same candidate simply overwrite it.
template <bool WRITE>
__global__ void __launch_bounds__(256) l1_wave_kernel(const uint64_t* __restrict__ hits, const uint64_t* __restrict__ read_hit_off,
                                                      const int32_t* __restrict__ read_len, const int32_t* __restrict__ min_hits, int64_t n_reads,
                                                      uint32_t* __restrict__ cand_n, const uint64_t* __restrict__ cand_off, int32_t* __restrict__ cand,
                                                      int32_t* __restrict__ cand_read, int32_t* __restrict__ cand_hint /* optional: seed hits inside the candidate */) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= n_reads) return;
  const uint64_t o = read_hit_off[r];
  const int64_t H = (int64_t)(read_hit_off[r + 1] - o);
  const int len = read_len[r];
  int m = min_hits[r]; if (m < 1) m = 1;                         // :349
  const uint64_t wbase = WRITE ? cand_off[r] : 0;
  int count = 0, prev_seq = -1, prev_wa = 0;
  int64_t open_i = 0;                                            // the hit that opened the candidate the previous chunk ended in
  for (int64_t base = 0; base + m <= H; base += 64) {
    const int64_t i = base + lane;
    const bool valid = i + m <= H;
    uint64_t a = 0, b = 0;
    if (valid) { a = hits[o + i]; b = hits[o + i + m - 1]; }
    const int sa = (int)(a >> 32), sb = (int)(b >> 32), wa = pw_wpos((uint32_t)a), wb = pw_wpos((uint32_t)b);
    const bool q = valid && sa == sb && wb - wa < len;           // :365
    const int cs = max(0, wb - len + 1);                         // :368
    const uint64_t qm = __ballot(q);
    const uint64_t below = qm & ((1ull << lane) - 1ull);
    const int pl = below ? 63 - __builtin_clzll(below) : 0;
    const int p_seq_l = __shfl(sa, pl, 64), p_wa_l = __shfl(wa, pl, 64);
    const int p_seq = below ? p_seq_l : prev_seq, p_wa = below ? p_wa_l : prev_wa;
    const bool brk = q && !(p_seq == sa && p_wa >= cs);          // :374-380
    const uint64_t bm = __ballot(brk);
    if (WRITE && q) {
      const int k = count + __popcll(bm & ((2ull << lane) - 1ull)) - 1;
      const uint64_t above = lane < 63 ? qm & ~((2ull << lane) - 1ull) : 0ull;
      const bool last = above == 0ull || ((bm >> (__builtin_ctzll(above))) & 1ull);
      int32_t* c = cand + 3 * (wbase + (uint64_t)k);
      if (brk) { c[0] = sa; c[1] = cs; cand_read[wbase + (uint64_t)k] = (int32_t)r; }
      if (last) c[2] = wa;
      if (last && cand_hint) {
        // the seed hits of the candidate: from the hit that opened it to the last hit of the last qualifying run — with --all nearly all of them
        // lie inside ONE read-length window, so this is about what K5 will find as the matched count of its best window (mm_l2z.hpp: the band it predicts)
        const uint64_t opened = bm & ((2ull << lane) - 1ull);
        const int64_t oi = opened ? base + (63 - __builtin_clzll(opened)) : open_i;
        cand_hint[wbase + (uint64_t)k] = (int32_t)min((int64_t)0x7fffffff, i + m - oi);
      }
    }
    if (bm) open_i = base + (63 - __builtin_clzll(bm));
    count += __popcll(bm);
    if (qm) { const int ll = 63 - __builtin_clzll(qm); prev_seq = __shfl(sa, ll, 64); prev_wa = __shfl(wa, ll, 64); }
  }
  if (!WRITE && lane == 0) cand_n[r] = (uint32_t)count;
}

// ---------------------------------------------------------------------------------------------------
// result compaction: accepted candidates -> mapping records, read order preserved
// ---------------------------------------------------------------------------------------------------
// sums of the per-candidate work counters: one atomic per counter per block
// K5 workgroups of the 10 kb class (sketch <= 3072), made on the device: per read, its candidates in groups of four (four-wave
// workgroups); a remainder of one or two goes to a two-wave workgroup.  The same lists came from a host loop before, ~0.85 ms per
// 10^5 reads of branch mispredictions with the device waiting.  Group order across workgroups of this kernel is arbitrary (results are
// indexed by candidate).  ctr: [0] four-wave groups, [1] two-wave groups, [2] reads with candidates left to the host's classes,
// [3] largest sketch among the grouped reads.
__global__ void __launch_bounds__(256) l2_group_kernel(const uint64_t* __restrict__ cand_off, const int32_t* __restrict__ sk_n, const int32_t* __restrict__ read_len,
                                                       int64_t n, int min_len_dense, int dense_from, int no_small,
                                                       int32_t* __restrict__ gA0, int32_t* __restrict__ gAn, int32_t* __restrict__ gS0, int32_t* __restrict__ gSn,
                                                       unsigned int* __restrict__ ctr) {
  __shared__ unsigned int bA, bS, bOther, bMax, baseA, baseS;
  if (threadIdx.x == 0) { bA = 0; bS = 0; bOther = 0; bMax = 0; }
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t c_lo = 0, c_hi = 0; int sr = 0; bool mine = false;
  if (r < n) {
    c_lo = cand_off[r]; c_hi = cand_off[r + 1]; sr = sk_n[r];
    const bool dense = sr >= dense_from && sr < L2_SKETCH_LIMIT && read_len[r] >= min_len_dense;
    mine = c_hi > c_lo && sr <= 3072 && !dense;
    if (c_hi > c_lo && !mine) atomicAdd(&bOther, 1u);
  }
  const unsigned ncr = mine ? (unsigned)(c_hi - c_lo) : 0u, nfull = ncr >> 2, rem = ncr & 3u;
  const bool rem_small = rem != 0 && rem <= 2 && !no_small;
  const unsigned a = nfull + ((rem != 0 && !rem_small) ? 1u : 0u), b = rem_small ? 1u : 0u;
  unsigned la = 0, ls = 0;
  if (a) la = atomicAdd(&bA, a);
  if (b) ls = atomicAdd(&bS, b);
  if (mine) atomicMax(&bMax, (unsigned)sr);
  __syncthreads();
  if (threadIdx.x == 0) {
    baseA = bA ? atomicAdd(&ctr[0], bA) : 0u; baseS = bS ? atomicAdd(&ctr[1], bS) : 0u;
    if (bOther) atomicAdd(&ctr[2], bOther);
    if (bMax) atomicMax(&ctr[3], bMax);
  }
  __syncthreads();
  for (unsigned g = 0; g < a; ++g) { gA0[baseA + la + g] = (int32_t)(c_lo + 4u * g); gAn[baseA + la + g] = (int32_t)min(4u, ncr - 4u * g); }
  if (b) { gS0[baseS + ls] = (int32_t)(c_lo + 4u * nfull); gSn[baseS + ls] = (int32_t)rem; }
}

// K5 workgroups in the order of where their first candidate lies (contig, start): the reads of a sample cover their genomes several times over,
// so workgroups that run at the same time then stream overlapping pieces of pos[] and meet them in L2 / the Infinity Cache (tools/k3_locality.py:
// K5 -5 % with the reads of the bench batch in mapped order; the order of the workgroups is free, results are indexed by candidate).
__global__ void __launch_bounds__(256) l2_group_keys_kernel(const int32_t* __restrict__ g0, const int32_t* __restrict__ gn, const int32_t* __restrict__ cand, int64_t n,
                                                           uint64_t* __restrict__ key, uint64_t* __restrict__ val) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n) return;
  const int32_t c0 = g0[g];
  key[g] = (uint64_t)(uint32_t)cand[3 * (int64_t)c0] << 32 | (uint32_t)cand[3 * (int64_t)c0 + 1];
  val[g] = (uint64_t)(uint32_t)c0 << 32 | (uint32_t)gn[g];
}
// the sorted (first candidate, count) pairs back into the two group arrays
__global__ void __launch_bounds__(256) l2_group_unpack_kernel(const uint64_t* __restrict__ val, int64_t n, int32_t* __restrict__ g0, int32_t* __restrict__ gn) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n) return;
  g0[g] = (int32_t)(val[g] >> 32); gn[g] = (int32_t)(uint32_t)val[g];
}

// The streamed range of every candidate (computeMap.hpp:466, :477) — first index entry at or beyond the candidate's start, first at or beyond its end + read length —
// one thread per candidate, both searches interleaved.  The zone kernel's waves did these searches themselves, one behind the other: eight dependent round trips in
// front of every candidate's stream (directory, bucket bounds, two 64-ary probes, twice).  Same lower bounds as contig_lower_bound_wpos (mm_l2.hpp).
__global__ void __launch_bounds__(256) l2_ranges_kernel(IndexView I, const int32_t* __restrict__ cand, const int32_t* __restrict__ cand_read, const int32_t* __restrict__ read_len,
                                                        int64_t n, int64_t* __restrict__ rng) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const int contig = cand[3 * c], rs = cand[3 * c + 1], re = cand[3 * c + 2];
  const int len = read_len[cand_read[c]];
  const int64_t cbeg = (int64_t)I.cstart[contig];
  const uint64_t d0 = I.dir_off[contig], nb = I.dir_off[contig + 1] - d0 - 1;
  const int t0 = rs, t1 = re + len;
  const uint64_t b0 = min((uint64_t)max(t0, 0) >> I.dir_shift, nb - 1), b1 = min((uint64_t)max(t1, 0) >> I.dir_shift, nb - 1);
  int64_t lo0 = cbeg + (int64_t)I.dir[d0 + b0], hi0 = cbeg + (int64_t)I.dir[d0 + b0 + 1];
  int64_t lo1 = cbeg + (int64_t)I.dir[d0 + b1], hi1 = cbeg + (int64_t)I.dir[d0 + b1 + 1];
  while (lo0 < hi0 || lo1 < hi1) {
    const int64_t m0 = lo0 < hi0 ? (lo0 + hi0) >> 1 : lo0, m1 = lo1 < hi1 ? (lo1 + hi1) >> 1 : lo1;
    const uint32_t p0 = I.pos[min(m0, I.N - 1)].pw, p1 = I.pos[min(m1, I.N - 1)].pw;
    if (lo0 < hi0) { if (pw_wpos(p0) < t0) lo0 = m0 + 1; else hi0 = m0; }
    if (lo1 < hi1) { if (pw_wpos(p1) < t1) lo1 = m1 + 1; else hi1 = m1; }
  }
  rng[2 * c] = lo0; rng[2 * c + 1] = max(lo0, lo1);
}

__global__ void __launch_bounds__(256) l2_stats_kernel(const L2Result* __restrict__ l2, int64_t n, unsigned long long* __restrict__ counters) {
  __shared__ unsigned long long acc[5];
  if (threadIdx.x < 5) acc[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long a = 0, b = 0, c = 0, d = 0, e = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) { a += l2[i].n_stream; b += l2[i].n_evals; c += l2[i].n_rebuilds; d += l2[i].pad2; e += (unsigned long long)l2[i].pad; }
  atomicAdd(&acc[0], a); atomicAdd(&acc[1], b); atomicAdd(&acc[2], c); atomicAdd(&acc[3], d); atomicAdd(&acc[4], e);
  __syncthreads();
  if (threadIdx.x < 3) atomicAdd(&counters[threadIdx.x], acc[threadIdx.x]);
  if (threadIdx.x == 3) atomicAdd(&counters[15], acc[3]);   // slide rounds (diagnostic)
  if (threadIdx.x == 4) atomicAdd(&counters[12], acc[4]);   // zone passes of the zone kernels (diagnostic)
}

__global__ void accept_flags_kernel(const L2Result* __restrict__ l2, int64_t n, uint32_t* __restrict__ flag) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flag[i] = l2[i].accepted ? 1u : 0u;
}
__global__ void write_records_kernel(const L2Result* __restrict__ l2, const int32_t* __restrict__ cand_read, const int32_t* __restrict__ sk_n,
                                     const uint32_t* __restrict__ flag, const uint64_t* __restrict__ rank, int64_t n,
                                     mm_map_record* __restrict__ rec) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !flag[i]) return;
  mm_map_record m;
  m.read = cand_read[i]; m.ref_contig = l2[i].contig; m.ref_start = l2[i].mean_pos; m.shared = l2[i].shared;
  m.sketch = sk_n[m.read]; m.strand = l2[i].strand; m.mapq = 0.0;
  rec[rank[i]] = m;
}
__global__ void read_rec_bounds_kernel(const uint64_t* __restrict__ cand_off, const uint64_t* __restrict__ rank, int64_t n_reads,
                                       uint64_t* __restrict__ rec_off) {
  int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r <= n_reads) rec_off[r] = rank[cand_off[r]];
}

}  // namespace mm
