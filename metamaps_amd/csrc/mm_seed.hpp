// K3 kernels — index probe, seed-hit gather and the exact seed-hit pre-filter (computeMap.hpp:307-323) — with the small copy /
// sum / bounds kernels beside them.  Included by mm_map.hip alone.
#pragma once
#include "mm_map.hpp"

namespace mm {

// ---------------------------------------------------------------------------------------------------
// K3  probe (one workgroup per read) and gather
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) probe_kernel(IndexView I, const uint32_t* __restrict__ sk_hash, const uint64_t* __restrict__ off,
                                                    const int32_t* __restrict__ sk_n, uint32_t* __restrict__ probe_cnt,
                                                    uint64_t* __restrict__ probe_start, const uint8_t* __restrict__ only /* optional: reads to do */) {
  // Four lanes per lookup, each reading one 16-byte slot of the hash's home sector (mm_index.hpp: tab_slot): one 64-byte
  // request resolves nearly every lookup; NP lookups per group in flight.
  const int r = blockIdx.x;
  if (only && !only[r]) return;
  const uint64_t o = off[r];
  const int s = sk_n[r];
  const int grp = threadIdx.x >> 2, sub = threadIdx.x & 3, gshift = (threadIdx.x & 63) & ~3;
  const ulonglong2* __restrict__ tab = reinterpret_cast<const ulonglong2*>(I.tab);
  const uint64_t tslots = (uint64_t)I.tab_buckets << 2;
  constexpr int NP = 4;                                          // lookups in flight per group
  for (int i0 = grp; i0 < s; i0 += 64 * NP) {
    uint32_t hq[NP]; uint64_t sq[NP]; ulonglong2 vq[NP];
#pragma unroll
    for (int u = 0; u < NP; ++u) { hq[u] = i0 + 64 * u < s ? sk_hash[o + i0 + 64 * u] : 0u; sq[u] = tab_slot(hq[u], I.tab_buckets); }
#pragma unroll
    for (int u = 0; u < NP; ++u) vq[u] = tab[sq[u] + sub];
    auto resolve = [&](uint32_t h, uint64_t slot, ulonglong2 v, bool active, int i) {
      bool pending = active;
      while (__any(pending)) {                                   // (wave-wide loop: the ballots below need every lane)
        const bool match = pending && v.x != 0 && (uint32_t)v.x == h, empty = pending && v.x == 0;
        const uint32_t gm = (uint32_t)(__ballot(match) >> gshift) & 0xfu, ge = (uint32_t)(__ballot(empty) >> gshift) & 0xfu;
        if (pending && (gm | ge)) {
          // slots are filled in probing order and never emptied: a match is the key's slot, an empty slot without one means absent
          if (match) {
            const uint32_t cnt = (uint32_t)(v.x >> 32);
            const bool keep = (uint64_t)cnt < (uint64_t)(int64_t)I.freq_threshold;   // computeMap.hpp:317
            probe_cnt[o + i] = keep ? cnt : 0u;
            probe_start[o + i] = keep ? v.y : 0ull;
          } else if (!gm && sub == 0) { probe_cnt[o + i] = 0u; probe_start[o + i] = 0ull; }
          pending = false;
        }
        if (pending) { slot = tab_next_sector(slot, tslots); v = tab[slot + sub]; }
      }
    };
#pragma unroll
    for (int u = 0; u < NP; ++u) resolve(hq[u], sq[u], vq[u], i0 + 64 * u < s, i0 + 64 * u);
  }
}

__global__ void __launch_bounds__(256) gather_hits_kernel(IndexView I, const uint64_t* __restrict__ off, const int32_t* __restrict__ sk_n,
                                                          const uint32_t* __restrict__ probe_cnt, const uint64_t* __restrict__ probe_start,
                                                          const uint64_t* __restrict__ hit_off, uint64_t* __restrict__ hits) {
  const int r = blockIdx.x;
  const uint64_t o = off[r];
  const int s = sk_n[r];
  for (int i = threadIdx.x; i < s; i += 256) {
    uint32_t c = probe_cnt[o + i];
    if (!c) continue;
    const uint64_t* src = I.occ + probe_start[o + i];
    uint64_t* dst = hits + hit_off[o + i];
    for (uint32_t j = 0; j < c; ++j) dst[j] = src[j] & ~(uint64_t)(PW_DP | PW_DN);
  }
}

// ---------------------------------------------------------------------------------------------------
// K3c  exact seed-hit pre-filter.  At miniSeq+H density the 32-bit hash space is saturated:
// a read draws ~10^4 chance hits scattered over the whole reference, and only hits that sit in a run of
// `minimumHits` hits of one contig spanning less than the read length can ever produce or shape an L1
// candidate (computeMap.hpp:357-385).  Positions are binned in 8192-base bins of the concatenated reference; a
// run shorter than the read touches at most nb = (len-1)/8192 + 2 consecutive bins, so a hit can be dropped when no
// window of nb consecutive bins around it holds minimumHits hits.  Bins are counted modulo 8192 bins in LDS
// (aliasing and contig borders only over-count, so nothing needed is lost).  Dropping hits that belong to no
// qualifying run leaves every qualifying run intact and cannot create a new one (a run that qualifies after
// dropping also qualifies before, so none of its members was dropped).
// The bin of every index entry is precomputed (occ16[], 2 bytes per entry, same layout as occ[]): both passes
// read a quarter of the list bytes, mostly one 64-byte sector per list, and only survivors touch occ[] itself.
// ---------------------------------------------------------------------------------------------------
// survivors are staged per read (8 B each, capacity 1024 + 2 x sketch size: stage_off); reads with more are re-filtered by the write kernel
// Two slot tables: 8 192 slots counted from the 13-bit codes of occ16[] (reads up to ~32 kb), and 32 768 slots counted from the
// entries of occ[] themselves (slot = position bin + a per-contig offset) for longer reads.  Chance hits grow with the read length and
// so does the window, so with 8 192 slots a 100 kb read (3.8*10^5 seed hits against the bench reference) has 650 hits in every
// window — above minimumHits everywhere, nothing is dropped, K4 sorts 1.5*10^9 hits per 4 000 reads; 32 768 slots keep the
// background a factor of four lower, below the threshold.  Any slot function that keeps neighbouring bins of a contig neighbours is
// a valid (superset) filter; pass 1 and the write pass of a read use the same table.  `cls[r]`: 0 fused kernel, 1 narrow, 2 wide.
template <int SLOT_BITS> struct HitFilterCfg {
  static constexpr int SLOTS = 1 << SLOT_BITS, THREADS = SLOTS / 32;
  static constexpr int EPL = SLOT_BITS == HF_SLOT_BITS_NARROW ? 8 : 2;   // entries per 16-byte load of a lane
  static constexpr int CLS = SLOT_BITS == HF_SLOT_BITS_NARROW ? 1 : 2;
  static constexpr size_t LDS = (size_t)SLOTS * 4 + (size_t)THREADS * 8 + 16;
};
template <bool WRITE, int SLOT_BITS>
__global__ void __launch_bounds__(HitFilterCfg<SLOT_BITS>::THREADS) hit_filter_kernel(IndexView I, const uint64_t* __restrict__ off, const int32_t* __restrict__ sk_n,
                                                         const uint32_t* __restrict__ probe_cnt, const uint64_t* __restrict__ probe_start,
                                                         const int32_t* __restrict__ read_len, const int32_t* __restrict__ min_hits,
                                                         uint32_t* __restrict__ surv_n, const uint64_t* __restrict__ read_hit_off,
                                                         uint64_t* __restrict__ hits, uint64_t* __restrict__ stage, const uint64_t* __restrict__ stage_off, int dbg,
                                                         const uint8_t* __restrict__ cls /* per read: which kernel filters it */,
                                                         uint32_t* __restrict__ raw_hits /* optional (WRITE = false): seed hits of the read before filtering */) {
  using Cfg = HitFilterCfg<SLOT_BITS>;
  constexpr int SLOTS = Cfg::SLOTS, THREADS = Cfg::THREADS, EPL = Cfg::EPL;
  constexpr bool NARROW = SLOT_BITS == HF_SLOT_BITS_NARROW;
  extern __shared__ __align__(16) uint32_t hf_lds[];
  uint32_t* const cnt = hf_lds;                                   // [SLOTS]
  uint32_t* const good = cnt + SLOTS;                             // [THREADS]
  uint32_t* const alive = good + THREADS;                         // [THREADS]
  uint32_t& cursor = alive[THREADS];
  const int r = blockIdx.x;
  const int my_cls = cls[r];
  if (!WRITE && my_cls != Cfg::CLS) return;
  if (WRITE && (my_cls == 2) != (Cfg::CLS == 2)) return;         // (reads of the fused kernel whose stage overflowed are re-filtered by the narrow kernel)
  if (WRITE) {                                                   // staged reads only need a copy
    const uint32_t n_s = surv_n[r];
    if (n_s <= (uint32_t)(stage_off[r + 1] - stage_off[r])) {
      if (dbg == 100 && n_s >= 2u && n_s <= 4096u) return;        // (dbg 100: the LDS radix sort takes these straight from the stage)
      const uint64_t wb = read_hit_off[r];
      for (uint32_t i = threadIdx.x; i < n_s; i += THREADS) hits[wb + i] = stage[stage_off[r] + i];
      return;
    }
  }
  const uint64_t o = off[r];
  const int s = sk_n[r];
  const uint32_t len = (uint32_t)max(read_len[r], 1);
  const int nb = min((int)((len - 1) >> HF_BIN_SHIFT) + 2, SLOTS);
  int m = min_hits[r]; if (m < 1) m = 1;
  for (int i = threadIdx.x; i < SLOTS; i += THREADS) cnt[i] = 0;
  if (threadIdx.x == 0) cursor = 0;
  __syncthreads();
  // One occurrence list per group of 4 lanes, one 16-byte load per lane (8 bin codes, or 2 entries): a list of up to 32 codes is a
  // single request of at most 64 bytes.  Random reads are bound by requests, not bytes (tools/ubench/randread), so the
  // lists of a group are software-pipelined: count/start three lists ahead, data two ahead.
  constexpr int GROUPS = THREADS / 4, PER_REQ = 4 * EPL;
  const int grp = threadIdx.x >> 2, sub = threadIdx.x & 3;
  // fn(c, st0, j0, v): lane `sub` of the group holds entries j0 + EPL*sub .. +EPL-1 of a list of c entries that starts
  // at occ[st0]; called by all lanes of the wave together (c == 0: nothing), so that fn may use wave-wide operations
  auto for_each_chunk = [&](auto&& fn) {
    auto meta = [&](int i, uint32_t& c, uint64_t& st0) { c = 0; st0 = 0; if (i < s) { c = probe_cnt[o + i]; st0 = probe_start[o + i]; } };
    auto issue = [&](uint32_t c, uint64_t st0, uint32_t j0, ulonglong2& v) {   // (clamped into the padded list)
      if (c) {
        const uint64_t e = st0 + min(j0 + (uint32_t)EPL * sub, (c - 1) & ~(uint32_t)(EPL - 1));
        v = NARROW ? *reinterpret_cast<const ulonglong2*>(I.occ16 + e) : *reinterpret_cast<const ulonglong2*>(I.occ + e);
      }
    };
    uint32_t c0, c1, c2, c3; uint64_t s0, s1, s2, s3;
    ulonglong2 v0 = make_ulonglong2(0, 0), v1 = v0, v2 = v0;
    meta(grp, c0, s0); meta(grp + GROUPS, c1, s1); meta(grp + 2 * GROUPS, c2, s2);
    issue(c0, s0, 0, v0); issue(c1, s1, 0, v1);
    for (int ib = 0; ib < s; ib += GROUPS) {                     // (wave-uniform trip count)
      meta(ib + grp + 3 * GROUPS, c3, s3);
      issue(c2, s2, 0, v2);
      fn(c0, s0, 0u, v0);
      for (uint32_t j0 = PER_REQ; __any(j0 < c0); j0 += PER_REQ) {   // long lists: the rest
        const uint32_t cl = j0 < c0 ? c0 : 0u;
        ulonglong2 v = make_ulonglong2(0, 0); issue(cl, s0, j0, v); fn(cl, s0, j0, v);
      }
      c0 = c1; s0 = s1; v0 = v1; c1 = c2; s1 = s2; v1 = v2; c2 = c3; s2 = s3;
    }
  };
  auto code_of = [](const ulonglong2& v, int t) -> uint32_t {
    if (NARROW) return (uint32_t)((t < 4 ? v.x : v.y) >> (16 * (t & 3))) & (uint32_t)(SLOTS - 1);
    const uint64_t e = t ? v.y : v.x;                            // contig << 32 | wpos << 3 | flags
    return (((uint32_t)e >> (3 + HF_BIN_SHIFT)) + (uint32_t)(e >> 32) * 40503u) & (uint32_t)(SLOTS - 1);
  };
  if (dbg == 2) {
    uint32_t a = 0;
    for_each_chunk([&](uint32_t c, uint64_t, uint32_t j0, const ulonglong2& v) { for (int t = 0; t < EPL; ++t) if (j0 + (uint32_t)EPL * sub + t < c) a += code_of(v, t); });
    if (a == 0x12345678u) cnt[0] = 1;
  } else for_each_chunk([&](uint32_t c, uint64_t, uint32_t j0, const ulonglong2& v) {
#pragma unroll
    for (int t = 0; t < EPL; ++t) if (j0 + (uint32_t)EPL * sub + t < c) atomicAdd(&cnt[code_of(v, t)], 1u);
  });
  __syncthreads();
  if (dbg == 1 || dbg == 2) { if (!WRITE && threadIdx.x == 0) surv_n[r] = 0; return; }   // timing aid (MM_HF_DBG): pass 1 only
  {
    // good[b]: the window of nb bins starting at b holds >= m hits (sliding sum over this thread's 32 window starts);
    // alive[b]: some good window contains b, i.e. good dilated by nb positions (all modulo the slot count)
    const int b0 = threadIdx.x * 32;
    uint32_t sum = 0, bits = 0;
    for (int i = 0; i < nb; ++i) sum += cnt[(b0 + i) & (SLOTS - 1)];
    for (int t = 0; t < 32; ++t) {
      bits |= (sum >= (uint32_t)m ? 1u : 0u) << t;
      sum += cnt[(b0 + t + nb) & (SLOTS - 1)] - cnt[(b0 + t) & (SLOTS - 1)];
    }
    good[threadIdx.x] = bits;
    __syncthreads();
    uint32_t al = 0;
    for (int j = 0; j < nb; ++j) {                               // bit b of alive = OR over j < nb of good bit (b - j)
      const int wsh = j >> 5, bsh = j & 31;
      const uint32_t g0 = good[(threadIdx.x - wsh) & (THREADS - 1)], g1 = good[(threadIdx.x - wsh - 1) & (THREADS - 1)];
      al |= bsh ? (g0 << bsh) | (g1 >> (32 - bsh)) : g0;
    }
    alive[threadIdx.x] = al;
    __syncthreads();
  }
  const uint64_t wbase = WRITE ? read_hit_off[r] : 0;
  const uint64_t stage_base = stage_off[r];
  const uint32_t stage_cap = (uint32_t)(stage_off[r + 1] - stage_base);
  uint64_t* const dst = WRITE ? hits + wbase : stage + stage_base;
  const uint32_t dst_cap = WRITE ? 0xffffffffu : stage_cap;
  // second pass: survivors (a few per cent) park the index of their entry, which is then replaced by the entry itself.
  // Per chunk the wave reserves its slots with one atomic (bit mask per lane, prefix sum across the wave) — a branch and
  // an atomic per surviving entry would serialise the wave on LDS round trips.
  const int lane = threadIdx.x & 63;
  for_each_chunk([&](uint32_t c, uint64_t st0, uint32_t j0, const ulonglong2& v) {
    const uint32_t e0 = j0 + (uint32_t)EPL * sub;
    uint32_t mask = 0;
#pragma unroll
    for (int t = 0; t < EPL; ++t) { const uint32_t b = code_of(v, t); mask |= ((e0 + t < c) ? (alive[b >> 5] >> (b & 31)) & 1u : 0u) << t; }
    if (dbg == 4) { if (mask == 0xdeadu) cnt[1] = 1; return; }   // timing aid: reads and bit tests only
    const int mine = __popc(mask);
    const int incl = wave_incl_scan(mine);
    const int total = __builtin_amdgcn_readlane(incl, 63);
    if (total == 0) return;
    uint32_t base = 0;
    if (lane == 63) base = atomicAdd(&cursor, (uint32_t)total);
    base = (uint32_t)__builtin_amdgcn_readlane((int)base, 63);
    uint32_t pos = base + (uint32_t)(incl - mine);
    while (mask) {
      const int t = __ffs(mask) - 1; mask &= mask - 1;
      if (pos < dst_cap) dst[pos] = st0 + e0 + t;
      ++pos;
    }
  });
  __syncthreads();
  const uint32_t n_s = min(cursor, dst_cap);
  if (dbg == 3 || dbg == 4) { if (!WRITE && threadIdx.x == 0) surv_n[r] = 0; return; }   // timing aid: without the fetch of the survivors
  for (uint32_t j = threadIdx.x; j < n_s; j += THREADS) dst[j] = I.occ[dst[j]] & ~(uint64_t)(PW_DP | PW_DN);
  if (!WRITE && threadIdx.x == 0) surv_n[r] = cursor;
  if (!WRITE && raw_hits) {                                      // (the bin counters still hold every hit of the read)
    __syncthreads();
    uint32_t acc = 0;
    for (int i = threadIdx.x; i < SLOTS; i += THREADS) acc += cnt[i];
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(&raw_hits[r], acc);
  }
}

// ---------------------------------------------------------------------------------------------------
// K3 + K3c fused for reads whose sketch and seed hits fit LDS (the 10 kb class): probe, count, filter in ONE launch.
// hit_filter_kernel above reads every occurrence list twice (count pass, then the pass that tests each entry against the
// surviving bins) and takes its list heads from arrays probe_kernel wrote to global memory.  Random requests, not bytes, are
// what these kernels pay for (tools/ubench/randread), so here every list is requested ONCE: a workgroup of 1024 threads keeps
// in LDS
//     the list heads (first occurrence, count) of the sketch          phase 0: table look-ups, 4 lanes per hash
//     the 13-bit bin codes of every seed hit, 8 per 16-byte piece      phase 1: one 16-byte load per piece, the pieces handed out
//                                                                      to the lanes; bins counted as they arrive
// and the second pass (phase 2) is bit tests over LDS; only survivors (a few per cent) touch occ[].  Results, staging and
// overflow protocol are those of hit_filter_kernel<false>: survivors staged per read, surv_n[r] their number.  A read that does
// not fit (sketch > SF_SMAX, more than SF_CHUNKS code pieces, more than 65 535 seed hits, or a full stage) is flagged in
// need_old[] and redone by probe_kernel + hit_filter_kernel, which skip every other read.
//
// The workgroup is resident and streams through the reads (one workgroup per CU, 158 KB of LDS; reads handed out by a ticket
// counter) and overlaps itself: the table look-ups of read r + 1 are in flight — their answers wait in registers, 11 x 16 bytes per
// lane — while read r tests its parked codes against the surviving bins, writes its survivor slots and fetches its survivors.
// (A read's phases one after the other, one workgroup per read: VALU 40 %, LDS 19 %, waiting on memory 26 % of the cycles,
// profiles/r02_sq_counters.txt.)
// What the form needs to work at all (each found in the ISA, docs/history.md section 4):
//   * the barriers of the loop are LDS-only (s_waitcnt lgkmcnt(0) + s_barrier): nothing may drain the vector memory counter
//     between the issue of the look-ups and their use;
//   * everything a read needs from global memory besides its lists comes through SCALAR loads (class byte, sketch size, offsets,
//     stage bounds, read length, minimumHits): a vector load behind the look-ups waits for them (the counter is in-order);
//   * values derived from the thread index are re-derived per iteration from a value the compiler cannot see through: hoisted out of
//     the loop they are spilled, and a reload from scratch is a vector memory operation;
//   * look-ups that need a second probe (a full home sector) are re-issued together, after all eleven answers have been looked at:
//     one more round trip per read instead of one per list of a lane group (2.4 ms of 15.6 in the first version).
// Results are those of the two-pass kernels hit for hit (tests/test_gpu_parity.py).
// ---------------------------------------------------------------------------------------------------
constexpr int SF_THREADS = 1024, SF_GROUPS = SF_THREADS / 4;
constexpr int SF_LPG = 11;                                      // lists per lane group
constexpr int SF_SMAX = SF_GROUPS * SF_LPG;                     // 2816 sketch hashes (reads up to ~12.5 kb at w = 8)
constexpr int SF_CHUNKS = 6144;                                 // parked code pieces (8 codes, 16 bytes each): 49 152 seed hits incl. padding
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// SF_STREAM_WAVES_PER_EU: the register budget of the streaming kernel.  4 (default) = all 512 registers of a SIMD's lane slot go to its four waves, 128
// each.  5 = 96 each, which leaves 128 per SIMD — one wave of another kernel — free beside the resident workgroup; together with the 11 KB of LDS
// that lstart8 freed (20 KB left: a minimizer workgroup of the OTHER worker's batch fits) VALU-bound work could run under this kernel's memory
// waits.  Measured in round 5 (tools/ab.sh, one box, in turns): at 96 registers 43 are spilled, and a reload from scratch waits behind the look-ups in
// flight: this kernel 14.9 -> 16.9 ms alone; the other worker's K1 does get in (its time inside the timed region 17 -> 13 ms), the step does not
// gain: 45.4 / 47.4 ms against 44.5 / 46.9.  Not adopted; the switch stays for the record (tools/ab_build.sh w5 "-DSF_STREAM_WAVES_PER_EU=5").
// (That was the 141 KB layout.  Since the round's last session the kernel keeps 32-bit counters and an anchor table: 158 KB of LDS, nothing fits beside it.)
#ifndef SF_STREAM_WAVES_PER_EU
#define SF_STREAM_WAVES_PER_EU 4
#endif
// The streaming kernel's LDS.  Round 5 (tools/sf_grid_sweep.py): this kernel's time follows the number of CUs at work (64 resident workgroups:
// 55.6 ms, 256: 15.2 ms — 13.9 ms x 4), i.e. it is bound by what a CU executes per read — 2 580 VALU instructions per wave and read, most of them
// in phase 1's count-and-park of the codes (per code: extract, validity test under its own branch, counter address and increment of a packed 16-bit
// pair; per piece: 28 instructions that spread the list number and the valid count over the spare bits) and their undoing in phase 2 — not by
// the memory side, which it loads to 80 % of its random-request ceiling.  So:
//   * the padding entries of occ16[] carry codes of their own (hf_pad_code, mm_index.hpp: 8192 + a number below 64), which land in 64 dummy
//     counters and are never alive: no valid count, no mask, no branch per code;
//   * counters are 32-bit words (address = code * 4, increment 1);
//   * a 16-byte piece is parked as it was loaded; the list a piece belongs to is found from anchor[] (the list of every fourth piece) and a
//     short walk over coff8[];
//   * phase 1 hands the PIECES out to the lanes (piece q to lane q mod 1024), not the lists to groups of four lanes with a second round for what
//     lies beyond a list's first 32 entries: the average list has 17 entries, so a third of the lanes had a piece to count, and an LDS atomic costs
//     what it costs per wave-instruction (6.0 cycles with every third lane active, 7.5 with all: tools/ubench/lds_rates) — 48 of them per wave and
//     read instead of 120, six loads per lane instead of fifteen, one round trip instead of two, and no table of further pieces to build.
struct SeedFilterStreamLds {
  uint32_t cnt[HF_SLOTS + HF_PAD_SLOTS];                        // hits per bin; the last 64: the padding entries' dummies
  uint32_t good[HF_SLOTS / 32], alive[HF_SLOTS / 32 + 4];       // alive[256 ..]: the pad codes' words, zero for the life of the workgroup
  uint32_t lstart8[SF_SMAX];                                    // first occurrence of every list / 8 (lists start on 64-byte sectors = multiples of 8 entries, padded_counts_kernel;
                                                                // an index of more than 2^35 padded occurrences — 275 GB of occ[] alone — does not fit a device)
  uint16_t lcnt[SF_SMAX];
  uint16_t coff8[SF_SMAX + 8];                                  // first code piece of every list (+ total)
  uint16_t anchor[SF_CHUNKS / 4];                               // the list piece 4 a belongs to
  uint32_t wsum[SF_THREADS / 64], wsum2[SF_THREADS / 64];
  uint32_t cursor, fallback, total8, hraw, tick[2], pad_[2];       // pad_[0]: the streaming kernel's group counter of phase 2
  ulonglong2 codes[SF_CHUNKS];                                  // 8 codes per piece, as loaded
};
static_assert(sizeof(SeedFilterStreamLds) <= 160 * 1024, "the streaming seed filter's LDS must fit one CU");
template <bool PROF>
__global__ void __launch_bounds__(SF_THREADS) __attribute__((amdgpu_waves_per_eu(SF_STREAM_WAVES_PER_EU, SF_STREAM_WAVES_PER_EU))) seed_filter_stream_kernel(IndexView I, const uint32_t* __restrict__ sk_hash, const uint64_t* __restrict__ off,
                                                                        const int32_t* __restrict__ sk_n, const int32_t* __restrict__ read_len,
                                                                        const int32_t* __restrict__ min_hits, uint32_t* __restrict__ surv_n,
                                                                        uint64_t* __restrict__ stage, const uint64_t* __restrict__ stage_off,
                                                                        uint8_t* need_old, const uint32_t* __restrict__ cls_words /* = need_old, read-only view */,
                                                                        uint32_t* __restrict__ raw_hits, int n_reads, uint32_t* __restrict__ ticket,
                                                                        unsigned long long* __restrict__ prof /* optional (MM_SF_PROF): cycles per phase, summed over the workgroups */) {
  extern __shared__ __align__(16) unsigned char sf_dyn[];
  SeedFilterStreamLds& L = *reinterpret_cast<SeedFilterStreamLds*>(sf_dyn);
  const ulonglong2* __restrict__ tab = reinterpret_cast<const ulonglong2*>(I.tab);
  const uint64_t tslots = (uint64_t)I.tab_buckets << 2;
  uint32_t hq[SF_LPG]; ulonglong2 vq[SF_LPG];                      // the look-ups in flight: hashes and home-sector slots of the NEXT read
  int r_cur = 0, s_cur = 0; uint64_t o_cur = 0;
  unsigned long long pt[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, pt0 = 0;
  auto lapp = [&](int i) { if (PROF) { const unsigned long long t = __builtin_readcyclecounter(); pt[i] += t - pt0; pt0 = t; } };
  if (PROF) pt0 = __builtin_readcyclecounter();
  
  for (int it = -1; it < 0 || r_cur < n_reads; ++it) {           // it = -1: the prologue (first ticket, first look-ups)
    int tid = (int)threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wid = tid >> 6;
    const int grp = tid >> 2, sub = tid & 3, gshift = lane & ~3;
    auto uni64 = [](uint64_t v) { return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32; };
    // class, sketch size and offset of read r: three independent scalar loads (cls_words aliases need_old read-only: the class byte of
    // read r is written by the host before the launch and by the workgroup that handles r; nobody else's view of it matters).
    // A read this kernel does not take (another class, or no sketch) comes back with s = 0.
    auto head = [&](int r, int& s, uint64_t& o) {
      const int rr = min(r, n_reads - 1);
      const uint32_t cw = cls_words[rr >> 2]; const int sn = sk_n[rr]; const uint64_t on = off[rr];
      s = 0; o = 0;
      if (r < n_reads && !((cw >> (8 * (rr & 3))) & 0xffu)) {
        s = sn; o = on;
        if (s <= 0) { s = 0; if (tid == 0) { surv_n[r] = 0; raw_hits[r] = 0; } }
      }
    };
    // (unconditional loads off a scalar base with 32-bit lane offsets, the index clamped into the sketch: a load under its own branch,
    // or one whose address registers are recycled, gets a vector-memory wait in front of it — eleven serial round trips; lanes beyond
    // the sketch look a valid hash up again and ignore the answer)
    auto load_hashes = [&](int s_, uint64_t o_) {
      const int su = __builtin_amdgcn_readfirstlane(s_);
      const char* __restrict__ hb = reinterpret_cast<const char*>(sk_hash + uni64(o_));
      const uint32_t last = (uint32_t)max(su - 1, 0);
      if (su > 0) {
#pragma unroll
        for (int u = 0; u < SF_LPG; ++u) hq[u] = *reinterpret_cast<const uint32_t*>(hb + (size_t)(min((uint32_t)(grp + SF_GROUPS * u), last) << 2));
      } else {
#pragma unroll
        for (int u = 0; u < SF_LPG; ++u) hq[u] = 0u;
      }
    };
    auto issue_lookups = [&]() {
#pragma unroll
      for (int u = 0; u < SF_LPG; ++u) asm volatile("" : "+v"(hq[u]));   // (the hashes are first used HERE: keeps the slot arithmetic, and the wait for the hash loads with it, from drifting up to the loads)
      int sub_ = (int)threadIdx.x & 3;
      asm volatile("" : "+v"(sub_));                               // (a value of its own: the lane's table address of the resolve step need not live — in scratch — until here)
#pragma unroll
      for (int u = 0; u < SF_LPG; ++u) vq[u] = tab[tab_slot(hq[u], I.tab_buckets) + sub_];
    };
    if (it < 0) {
      if (tid == 0) L.tick[0] = atomicAdd(ticket, 1u);
      if (tid < 4) L.alive[HF_SLOTS / 32 + tid] = 0;              // (the pad codes' bins: never alive)
      lds_barrier();
      r_cur = __builtin_amdgcn_readfirstlane((int)L.tick[0]);
      head(r_cur, s_cur, o_cur);
      load_hashes(s_cur, o_cur);
      issue_lookups();
      continue;
    }
    if (tid == 0) L.tick[(it + 1) & 1] = atomicAdd(ticket, 1u);   // the read after this one (read by all after the next barrier)
    int r_next = n_reads, s_next = 0; uint64_t o_next = 0;
    bool next_issued = false, next_known = false;
    if (s_cur > 0) {
      const int r = __builtin_amdgcn_readfirstlane(r_cur), s = __builtin_amdgcn_readfirstlane(s_cur);
      // what phase 2 needs of the read, fetched now (scalar loads)
      const uint64_t stage_base = stage_off[r];
      const uint32_t stage_cap = (uint32_t)(stage_off[r + 1] - stage_base);
      const uint32_t len = (uint32_t)max(read_len[r], 1);
      const int nb = min((int)((len - 1) >> HF_BIN_SHIFT) + 2, HF_SLOTS);
      int m = min_hits[r]; if (m < 1) m = 1;
      {
        uint32_t z = 0;
        asm volatile("" : "+v"(z));                                // (a zero made here: hoisted out of the loop, a register pair of zeros is kept in scratch, and its reload waits for the look-ups)
        for (int i = tid; i < (HF_SLOTS + HF_PAD_SLOTS) / 4; i += SF_THREADS) reinterpret_cast<uint4*>(L.cnt)[i] = make_uint4(z, z, z, z);
        if (tid < (int)(sizeof L.lcnt / 16)) reinterpret_cast<uint4*>(L.lcnt)[tid] = make_uint4(z, z, z, z);
        if (tid == 0) { L.cursor = z; L.fallback = z; L.pad_[0] = z; }
      }
      lds_barrier();
      lapp(0);
      // the next read's ticket is visible: its class, sketch size and offset are on their way while this read's look-ups are resolved
      r_next = __builtin_amdgcn_readfirstlane((int)L.tick[(it + 1) & 1]);
      head(r_next, s_next, o_next);
      next_known = true;
      // ---- phase 0: resolve the look-ups issued during the previous read.  Round 0 looks at all eleven answers and re-issues, for the
      // lane groups whose home sector was full without a match, the next sector; round 1 (rarely 2) looks at those.
      // pass 1: every answer looked at once; a lane group whose home sector is full without a match asks for the next sector — all such
      // requests of the lane are in flight together; pass 2 takes them up (and probes on, one sector at a time, in the rare case)
      // (lcnt[] is zero from the top of the iteration: only a hash that is found and kept writes its list; absent or cut by freqThreshold = no list)
      auto settle = [&](int i, uint32_t h, const ulonglong2& v, bool pending) -> bool {   // true: the look-up of this lane group is done
        // slots are filled in probing order and never emptied: a match is the key's slot, an empty slot without one means absent
        const bool match = pending && v.x != 0 && (uint32_t)v.x == h, empty = pending && v.x == 0;
        const uint32_t done = (uint32_t)(__ballot(match || empty) >> gshift) & 0xfu;
        if (match) {
          const uint32_t cnt = (uint32_t)(v.x >> 32);
          if ((uint64_t)cnt < (uint64_t)(int64_t)I.freq_threshold) {   // computeMap.hpp:317
            if (cnt > 0xffffu) L.fallback = 1;                    // (a list this long overflows the code area anyway)
            L.lcnt[i] = (uint16_t)cnt; L.lstart8[i] = (uint32_t)(v.y >> 3);
          }
        }
        return !pending || done != 0;
      };
      uint32_t pmask = 0;
#pragma unroll
      for (int u = 0; u < SF_LPG; ++u) {
        const int i = grp + SF_GROUPS * u;
        if (!settle(i, hq[u], vq[u], i < s)) { pmask |= 1u << u; vq[u] = tab[tab_next_sector(tab_slot(hq[u], I.tab_buckets), tslots) + sub]; }
      }
      lapp(7);                                                    // (first answers looked at, second probes issued)
      if (__any(pmask != 0)) {
#pragma unroll
        for (int u = 0; u < SF_LPG; ++u) {
          const int i = grp + SF_GROUPS * u;
          const uint32_t h = hq[u]; uint64_t slot = tab_next_sector(tab_slot(h, I.tab_buckets), tslots); ulonglong2 v = vq[u];
          bool pending = (pmask >> u) & 1u;
          while (__any(pending)) {
            if (settle(i, h, v, pending)) pending = false;
            if (pending) { slot = tab_next_sector(slot, tslots); v = tab[slot + sub]; }
          }
        }
      }
      lds_barrier();
      lapp(1);
      // ---- code piece offsets
      {
        uint32_t c8[3], hr = 0, mine = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) { const int i = tid * 3 + j; const uint32_t c = i < s ? L.lcnt[i] : 0u; c8[j] = (c + 7) >> 3; mine += c8[j]; hr += c; }
        const uint32_t inc = (uint32_t)wave_incl_scan((int)mine), inc2 = (uint32_t)wave_incl_scan((int)hr);
        if (lane == 63) { L.wsum[wid] = inc; L.wsum2[wid] = inc2; }
        lds_barrier();
        uint32_t basew = 0, tot = 0, tot2 = 0;
#pragma unroll
        for (int q = 0; q < SF_THREADS / 64; ++q) { const uint32_t x = L.wsum[q]; if (q < wid) basew += x; tot += x; tot2 += L.wsum2[q]; }
        uint32_t ex = basew + inc - mine;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int i = tid * 3 + j;
          if (i <= s) L.coff8[i] = (uint16_t)min(ex, 0xffffu);
          for (uint32_t a = (ex + 3) >> 2, a1 = min((ex + c8[j] + 3) >> 2, (uint32_t)(SF_CHUNKS / 4)); a < a1; ++a) L.anchor[a] = (uint16_t)i;   // pieces 4 a of this list
          ex += c8[j];
        }
        if (tid == 0) { L.total8 = tot; L.hraw = tot2; if (tot > (uint32_t)SF_CHUNKS || tot2 > 65535u) L.fallback = 1; }
      }
      lds_barrier();
      lapp(2);
      if (L.fallback) { if (tid == 0) { need_old[r] = 1; surv_n[r] = 0; raw_hits[r] = 0; } }
      else {
        // the next read's hashes: requested here, in front of the pieces (six pieces in flight leave the registers for them): they are there
        // long before the look-ups are issued behind the window sums
        load_hashes(s_next, o_next);
        // ---- phase 1: every 16-byte piece of every list once: piece q to lane q mod 1024, all loads of a lane in flight together, then all
        // eight codes of a piece counted (the pads behind a list's last entry in their dummies) and the piece parked as it is
        {
          constexpr int NP = SF_CHUNKS / SF_THREADS;
          const uint32_t T8u = (uint32_t)__builtin_amdgcn_readfirstlane((int)L.total8);
          ulonglong2 v[NP];
#pragma unroll
          for (int j = 0; j < NP; ++j) {
            v[j] = make_ulonglong2(0, 0);
            if ((uint32_t)(j * SF_THREADS) < T8u) {                // (wave-uniform; lanes beyond the last piece ask for it again and drop the answer)
              const uint32_t q = min((uint32_t)(tid + j * SF_THREADS), T8u - 1);
              uint32_t li = L.anchor[q >> 2];
              while ((uint32_t)L.coff8[li + 1] <= q) ++li;
              v[j] = *reinterpret_cast<const ulonglong2*>(I.occ16 + ((uint64_t)L.lstart8[li] << 3) + (uint64_t)(q - (uint32_t)L.coff8[li]) * 8u);
            }
          }
#pragma unroll
          for (int j = 0; j < NP; ++j) {
            const uint32_t q = (uint32_t)(tid + j * SF_THREADS);
            if (q < T8u) {
              const ulonglong2 x = v[j];
#pragma unroll
              for (int t = 0; t < 8; ++t) atomicAdd(&L.cnt[(uint32_t)((t < 4 ? x.x : x.y) >> (16 * (t & 3))) & 0xffffu], 1u);
              L.codes[q] = x;
            }
          }
          lapp(8);                                                 // (all pieces loaded, counted and parked)
        }
        lds_barrier();
        lapp(3);
        {
          // good[b] = the nb bins from b on hold minimumHits hits.  A lane takes the bins tid, tid + 1024, ...: neighbouring lanes read neighbouring
          // counters (eight consecutive bins per lane — the sliding form — put the 64 lanes of a read on four LDS banks), and a wave's 64 answers are one ballot
          const uint32_t* cnt = L.cnt;
#pragma unroll
          for (int kk = 0; kk < HF_SLOTS / SF_THREADS; ++kk) {
            const int b = tid + kk * SF_THREADS;
            uint32_t sum = 0;
            for (int i = 0; i < nb; ++i) sum += cnt[(b + i) & (HF_SLOTS - 1)];
            const uint64_t gb = __ballot(sum >= (uint32_t)m);
            if (lane == 0) { L.good[(b >> 5)] = (uint32_t)gb; L.good[(b >> 5) + 1] = (uint32_t)(gb >> 32); }
          }
        }
        lds_barrier();
        lapp(9);                                                   // (window sums)
        if (tid < HF_SLOTS / 32) {
          uint32_t al = 0;
          for (int j = 0; j < nb; ++j) {
            const int wsh = j >> 5, bsh = j & 31;
            const uint32_t g0 = L.good[(tid - wsh) & 255], g1 = L.good[(tid - wsh - 1) & 255];
            al |= bsh ? (g0 << bsh) | (g1 >> (32 - bsh)) : g0;
          }
          L.alive[tid] = al;
        }
        lapp(10);                                                  // (alive)
        lds_barrier();
        lapp(4);
        // The next read's home sectors: in flight from here to the top of the next iteration.  Issued BEHIND the barrier that publishes alive[] (round 6; until then in front
        // of it): the look-ups leave a CU at the rate its address path takes them (2 816 sectors, the kernel's bound), and a wave whose eleven are out goes on to
        // the bit tests instead of waiting at the barrier for the last wave's — the step 38.9-39.5 -> 36.4-38.2 ms in turns on one box, this kernel 12.6-13.1 -> 11.9-12.6 ms
        // (profiles/r06_ab_k3_barrier_first.txt).
        issue_lookups();
        lapp(11);                                                  // (hashes arrived, look-ups issued)
        next_issued = true;
        // ---- phase 2: bit tests over the parked codes
        uint64_t* const dst = stage + stage_base;
        uint16_t* const sv = reinterpret_cast<uint16_t*>(L.cnt);   // (2 x 8 256 slots: stage_cap = 1024 + 2 x sketch size <= 6 656, unless the test hook MM_HF_STAGE_CAP says otherwise)
        const uint32_t sv_cap = min(stage_cap, (uint32_t)(2 * (HF_SLOTS + HF_PAD_SLOTS)));
        const uint32_t T8 = L.total8;
        // Groups of 64 pieces handed out by a counter (round 6; until then piece q0 + tid for q0 = 0, 1 024, ...): the waves reach this phase one after the other — each
        // as its look-ups are out — and a wave that comes early takes more groups instead of waiting at the barrier behind the phase for the wave that comes last
        // (that barrier: 14 % of the kernel's cycles -> 1 %; the kernel 12.45 -> 12.16 ms over three alternations on one box).  The order of the survivor slots was
        // already the order in which the waves reach the cursor.
        uint32_t cv = 0;
        if (lane == 0) cv = atomicAdd(&L.pad_[0], 1u);
        for (uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)cv); c * 64u < T8; c = (uint32_t)__builtin_amdgcn_readfirstlane((int)cv)) {
          if (lane == 0) cv = atomicAdd(&L.pad_[0], 1u);         // (the next group: asked for before this one is worked on)
          const uint32_t q = c * 64u + (uint32_t)lane;
          uint32_t mask = 0;
          if (q < T8) {
            const ulonglong2 x = L.codes[q];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
              const uint32_t code = (uint32_t)((t < 4 ? x.x : x.y) >> (16 * (t & 3))) & 0xffffu;   // (a pad: one of the bins nothing is alive in)
              mask |= ((L.alive[code >> 5] >> (code & 31)) & 1u) << t;
            }
          }
          const int mine = __popc(mask);
          const int incl = wave_incl_scan(mine);
          const int total = __builtin_amdgcn_readlane(incl, 63);
          if (total == 0) continue;
          uint32_t base = 0;
          if (lane == 63) base = atomicAdd(&L.cursor, (uint32_t)total);
          base = (uint32_t)__builtin_amdgcn_readlane((int)base, 63);
          uint32_t pos = base + (uint32_t)(incl - mine);
          while (mask) {                                           // a survivor is noted as piece << 3 | entry, 16 bits, where the counters were (they are done with)
            const int t = __ffs(mask) - 1; mask &= mask - 1;
            if (pos < sv_cap) sv[pos] = (uint16_t)(q << 3 | (uint32_t)t);
            ++pos;
          }
        }
        lapp(12);                                                  // (bit tests, survivors noted)
        lds_barrier();
        lapp(5);
        const uint32_t n_s = L.cursor;
        if (n_s > sv_cap) { if (tid == 0) { need_old[r] = 1; surv_n[r] = 0; raw_hits[r] = 0; } }   // stage too small: the two-pass kernels redo the read
        else {
          // the occurrence of every survivor: list start + position in the list (the list of a piece: from the anchor of its group of four,
          // past the lists that end at or before it).  Noted in global memory and read back behind a full barrier, as until round 5, this
          // cost a store, a round trip and a wait for the look-ups in flight before the occurrences could even be asked for.
          for (uint32_t j = tid; j < n_s; j += SF_THREADS) {
            const uint32_t e = sv[j], q = e >> 3;
            uint32_t li = L.anchor[q >> 2];
            while ((uint32_t)L.coff8[li + 1] <= q) ++li;
            dst[j] = I.occ[((uint64_t)L.lstart8[li] << 3) + (uint64_t)(q - (uint32_t)L.coff8[li]) * 8u + (e & 7u)] & ~(uint64_t)(PW_DP | PW_DN);
          }
          if (tid == 0) { surv_n[r] = n_s; raw_hits[r] = L.hraw; }
        }
      }
    }
    if (!next_issued) {                                          // a read that was skipped or fell back: nothing to hide the look-ups behind
      lds_barrier();
      if (!next_known) { r_next = __builtin_amdgcn_readfirstlane((int)L.tick[(it + 1) & 1]); head(r_next, s_next, o_next); }
      load_hashes(s_next, o_next);
      issue_lookups();
    }
    lds_barrier();                                               // the LDS areas are free for the next read
    lapp(6);
    r_cur = r_next; s_cur = s_next; o_cur = o_next;
  }
  if (PROF && threadIdx.x == 0) for (int i = 0; i < 16; ++i) atomicAdd(&prof[i], pt[i]);
}

// range blockIdx.x of src, [sb, se), goes to dst starting at db
__global__ void __launch_bounds__(256) move_ranges_kernel(const uint64_t* __restrict__ src, const uint64_t* __restrict__ sb, const uint64_t* __restrict__ se,
                                                          uint64_t* __restrict__ dst, const uint64_t* __restrict__ db) {
  const uint64_t s0 = sb[blockIdx.x], n = se[blockIdx.x] - s0, d0 = db[blockIdx.x];
  for (uint64_t i = threadIdx.x; i < n; i += 256) dst[d0 + i] = src[s0 + i];
}
// sum of the probe counts (= raw seed hits of the batch); the filter path needs no per-list offsets, only this total
__global__ void __launch_bounds__(256) sum_u32_kernel(const uint32_t* __restrict__ v, int64_t n, unsigned long long* __restrict__ out) {
  unsigned long long acc = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) acc += v[i];
  for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d, 64);
  if ((threadIdx.x & 63) == 0 && acc) atomicAdd(out, acc);
}

// debug tap (mm_debug_probed_lists): how long are the occurrence lists the sketches of a batch ask for?  One thread per sketch hash;
// hist[0] = hash not in the index, hist[c] = lists of c entries (c < nb - 2), hist[nb - 2] = longer lists that are kept,
// hist[nb - 1] = lists cut by freqThreshold (computeMap.hpp:317)
__global__ void __launch_bounds__(256) probed_list_hist_kernel(IndexView I, const uint32_t* __restrict__ sk_hash, const uint64_t* __restrict__ off,
                                                               const int32_t* __restrict__ sk_n, int nb, unsigned long long* __restrict__ hist) {
  const int r = blockIdx.x, s = sk_n[r];
  const uint64_t o = off[r];
  for (int i = threadIdx.x; i < s; i += 256) {
    uint32_t cnt = 0; uint64_t start = 0;
    int b = 0;
    if (index_find(I, sk_hash[o + i], &cnt, &start)) b = (uint64_t)cnt < (uint64_t)(int64_t)I.freq_threshold ? (int)min(cnt, (uint32_t)(nb - 2)) : nb - 1;
    atomicAdd(&hist[b], 1ull);
  }
}

__global__ void read_hit_bounds_kernel(const uint64_t* __restrict__ off, const uint64_t* __restrict__ hit_off, int64_t n,
                                       uint64_t* __restrict__ read_hit_off) {
  int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r <= n) read_hit_off[r] = hit_off[off[r]];
}

}  // namespace mm
