// Shared host/device definitions of libmetamaps_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <deque>
#include <vector>
#include <stdexcept>
#include <memory>
#include <chrono>
#include <map>
#include <iterator>
#include <mutex>
#include <atomic>
#include <algorithm>
#include "../../include/metamaps_hip.h"
#include "mm_slab.hpp"
#include "task_pool.hpp"
#include "cpu_budget.hpp"

namespace mm {

// ---- error plumbing: internal code throws, the C ABI layer converts to a status + message ----------
struct Error : std::runtime_error {
  int status;
  Error(int st, const std::string& m) : std::runtime_error(m), status(st) {}
};
#define MM_HIP(expr)                                                                         \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess)                                                                    \
      throw mm::Error(_e == hipErrorOutOfMemory ? MM_ERR_NOMEM : MM_ERR_DEVICE,              \
                      std::string(#expr) + ": " + hipGetErrorString(_e));                    \
  } while (0)
#define MM_REQUIRE(cond, st, msg) \
  do { if (!(cond)) throw mm::Error((st), (msg)); } while (0)
#define MM_KERNEL_CHECK() MM_HIP(hipGetLastError())

}  // namespace mm
#include "mm_alloc.hpp"   // waits for a stream (mm_stream.hpp), device memory, DBuf
namespace mm {

// ---- index / minimizer record ------------------------------------------------------------------------
// One winnowed minimizer = 8 bytes: {hash, pw}.  pw packs window position, strand and two duplicate
// flags the index builder fills in (DESIGN.md §Data layout):
//   bit 0      strand (1 = FWD, 0 = REV)                      base_types.hpp:121-125
//   bit 1      DP: an earlier entry of the same contig carries the same hash
//   bit 2      DN: a later   entry of the same contig carries the same hash
//   bits 3..31 wpos (< 2^29: contigs up to 536 Mbp)
struct Rec { uint32_t hash; uint32_t pw; };
constexpr uint32_t PW_STRAND = 1u, PW_DP = 2u, PW_DN = 4u;
constexpr int PW_SHIFT = 3;
constexpr int64_t MAX_SEQ_LEN = (1LL << 29) - 1;
__host__ __device__ inline int32_t pw_wpos(uint32_t pw) { return (int32_t)(pw >> PW_SHIFT); }
__host__ __device__ inline int32_t pw_strand(uint32_t pw) { return (pw & PW_STRAND) ? 1 : -1; }

// ---- MurmurHash3_x64_128 low 32 bits, seed 42 (murmur3.h:226-303, commonFunc.hpp:33,71-81) -----------
__host__ __device__ inline uint64_t rotl64(uint64_t v, int r) { return (v << r) | (v >> (64 - r)); }
__host__ __device__ inline uint64_t fmix64(uint64_t v) {
  v ^= v >> 33; v *= 0xff51afd7ed558ccdULL;
  v ^= v >> 33; v *= 0xc4ceb9fe1a85ec53ULL;
  v ^= v >> 33;
  return v;
}
constexpr uint64_t MUR_C1 = 0x87c37b91114253d5ULL, MUR_C2 = 0x4cf5ad432745937fULL;
constexpr uint32_t MUR_SEED = 42u;

// k == 16: exactly one block (lo = bytes 0..7, hi = bytes 8..15, little endian), no tail
__host__ __device__ inline uint32_t murmur16(uint64_t lo, uint64_t hi) {
  uint64_t a = MUR_SEED, b = MUR_SEED;
  lo *= MUR_C1; lo = rotl64(lo, 31); lo *= MUR_C2; a ^= lo;
  a = rotl64(a, 27); a += b; a = a * 5 + 0x52dce729;
  hi *= MUR_C2; hi = rotl64(hi, 33); hi *= MUR_C1; b ^= hi;
  b = rotl64(b, 31); b += a; b = b * 5 + 0x38495ab5;
  a ^= 16; b ^= 16;
  a += b; b += a;
  a = fmix64(a); b = fmix64(b);
  a += b;
  return (uint32_t)a;
}
// general k (bytes need not be aligned); `rev` reads the bytes backwards from p (p points at the LAST byte)
template <bool REV>
__host__ __device__ inline uint32_t murmur_bytes(const uint8_t* p, int k) {
  auto at = [&](int i) -> uint64_t { return REV ? p[-i] : p[i]; };
  uint64_t a = MUR_SEED, b = MUR_SEED;
  int nb = k >> 4;
  for (int blk = 0; blk < nb; ++blk) {
    uint64_t lo = 0, hi = 0;
    for (int j = 0; j < 8; ++j) { lo |= at(16 * blk + j) << (8 * j); hi |= at(16 * blk + 8 + j) << (8 * j); }
    lo *= MUR_C1; lo = rotl64(lo, 31); lo *= MUR_C2; a ^= lo;
    a = rotl64(a, 27); a += b; a = a * 5 + 0x52dce729;
    hi *= MUR_C2; hi = rotl64(hi, 33); hi *= MUR_C1; b ^= hi;
    b = rotl64(b, 31); b += a; b = b * 5 + 0x38495ab5;
  }
  int rem = k & 15, base = nb << 4;
  uint64_t lo = 0, hi = 0;
  for (int j = 8; j < rem; ++j) hi |= at(base + j) << (8 * (j - 8));
  if (rem > 8) { hi *= MUR_C2; hi = rotl64(hi, 33); hi *= MUR_C1; b ^= hi; }
  for (int j = 0; j < rem && j < 8; ++j) lo |= at(base + j) << (8 * j);
  if (rem > 0) { lo *= MUR_C1; lo = rotl64(lo, 31); lo *= MUR_C2; a ^= lo; }
  a ^= (uint64_t)k; b ^= (uint64_t)k;
  a += b; b += a;
  a = fmix64(a); b = fmix64(b);
  a += b;
  return (uint32_t)a;
}

__host__ __device__ inline uint8_t ascii_of_code(uint32_t c) {      // 0,1,2,3 -> A,C,G,T
  return (uint8_t)(0x41 + 2 * (c & 1) + 6 * (c >> 1) + 11 * ((c & 1) & (c >> 1)));
}
__host__ __device__ inline uint8_t complement_ascii(uint8_t c) {    // commonFunc.hpp:38-55
  return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
}

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace mm

// ---- opaque handle bodies ----------------------------------------------------------------------------
struct mm_ctx {
  int device = -1;
  hipStream_t stream = nullptr;
  // A second stream for ONE purpose: the two launches of K5's 10 kb class (four-wave and two-wave workgroups, independent candidates) run side by side,
  // forked from and joined back into `stream` by events — everything else of a context stays on its one stream (the caching allocator relies on that;
  // the buffers the two launches touch are allocated before the fork and live past the join).  Created at first use.
  hipStream_t aux_stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  void aux_ready() {
    if (aux_stream) return;
    MM_HIP(hipStreamCreateWithFlags(&aux_stream, hipStreamNonBlocking));
    mm::stream_event_register(aux_stream);
    MM_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    MM_HIP(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
  }
  mm::DevAlloc alloc;
  std::string err;
  int cus = 0;
  void* comm = nullptr;          // ncclComm_t
  bool comm_shared = false;      // the communicator belongs to another context of this device (mm_comm_share)
  int comm_rank = 0, comm_size = 1;
  // per-(k, pi) cache of the host statistics thresholds (pure functions of the sketch size), mm_stats.hpp
  std::shared_ptr<void> lut_cache;
  int lut_k = 0; float lut_pi = 0;
  // K5 scratch kept across batches: the zone kernels' matched lists (mm_l2z.hpp), and the class masks of the zone kernels and of l2_kernel
  mm::GrowBuf l2_lists, l2_masks;
  // pinned bounce buffer for result downloads into caller-owned (pageable) memory
  void* pinned = nullptr; size_t pinned_bytes = 0;
  // pinned staging buffer of sequence uploads (mm_seq.hip: the 2-bit words are packed straight into it), and the threads that pack
  void* pinned_up = nullptr; size_t pinned_up_bytes = 0;
  std::unique_ptr<TaskPool> pack_pool;
  void* pinned_up_at_least(size_t bytes) {
    if (bytes > pinned_up_bytes) {
      if (pinned_up) { MM_HIP(mm::stream_sync(stream)); (void)hipHostFree(pinned_up); }
      pinned_up = nullptr; pinned_up_bytes = 0;
      const size_t want = bytes + bytes / 8;
      MM_HIP(hipHostMalloc(&pinned_up, want, hipHostMallocDefault));
      pinned_up_bytes = want;
    }
    return pinned_up;
  }
  void* pinned_at_least(size_t bytes) {
    if (bytes > pinned_bytes) {
      if (pinned) (void)hipHostFree(pinned);
      pinned = nullptr; pinned_bytes = 0;
      size_t want = bytes + bytes / 2 + (1 << 20);
      MM_HIP(hipHostMalloc(&pinned, want, hipHostMallocDefault));
      pinned_bytes = want;
    }
    return pinned;
  }
};

struct mm_seqset {
  mm_ctx* ctx = nullptr;
  bool frozen = false;
  bool hpc = false;                                             // a result of mm_seqset_hpc: the bases are not the sequences' own (mm_reads_encode refuses it)
  // host staging (until upload)
  std::deque<std::string> owned;                                // copies made by mm_seqset_add (stable addresses)
  std::vector<std::pair<const char*, size_t>> staged;           // what upload packs: views into `owned` or into caller memory (mm_seqset_add_view)
                                                                // or, for a set of BAM's 4-bit codes (mm_seqset_add_nt16), (codes, bases)
  std::vector<uint8_t> staged_rev;                              // nt16 only: 1 = the record is the reverse complement of the read
  int staged_kind = 0;                                          // 0 nothing staged yet, 1 ASCII, 2 nt16: one set holds one kind
  struct StagedQual { const uint8_t* p = nullptr; int offset = 0; bool set = false; };
  std::vector<StagedQual> staged_qual;                          // mm_seqset_add_qual: the viewed quality bytes of staged[i] (shorter than `staged`: the rest have none)
  struct StagedMods {                                           // mm_seqset_add_mods: copies of the groups of the sequences `seq` (ascending) that got a call
    std::vector<int32_t> seq; std::vector<int64_t> goff{0}, soff{0};   // groups [goff[r], goff[r + 1]) of seq[r]; skips and ML bytes [soff[g], soff[g + 1]) of group g
    std::vector<uint8_t> base, mode, ml; std::vector<int8_t> code; std::vector<uint32_t> skips;
  } staged_mods;
  // host-side metadata (always valid after upload / synthesis)
  std::vector<int32_t> len;            // per sequence
  std::vector<uint64_t> base;          // [n+1] first base of sequence i in the packed stream (multiple of 16)
  int64_t total_bases = 0;
  // device
  mm::DBuf<uint32_t> packed;           // 16 bases per word, base b at bits [2b, 2b+2)
  mm::DBuf<uint64_t> d_base;           // [n+1]
  mm::DBuf<int32_t> d_len;             // [n]
  mm::DBuf<uint64_t> exc_start;        // exception runs, sorted by start (stream coordinates)
  mm::DBuf<uint32_t> exc_len;
  mm::DBuf<uint8_t> exc_byte;
  int64_t n_exc = 0;
  // the quality plane (mm_seqset_add_qual; absent unless has_qual): byte base[i] + p is the Phred value 0..93 of base p of sequence i, 0xFF for "no
  // quality" (a sequence added without qualities, and the padding)
  bool has_qual = false;
  mm::DBuf<uint8_t> qual;              // [base[n]]: every base[i] is a multiple of 16 and the buffer starts on a 4-byte boundary, so the aligned 4-byte word that
                                       // holds any byte of sequence i lies inside [base[i], base[i + 1]) (mm_reads_out.hip reads the plane by such words)
  const uint8_t* qual_ptr() const { return has_qual ? qual.p : nullptr; }
  // the modification plane (mm_seqset_add_mods; absent unless has_mods): word base[i] + p is who | prob << 8 of base p of sequence i (mm_mods_core.hpp),
  // 0 for "no call" (a sequence added without groups, and the padding)
  bool has_mods = false;
  mm::DBuf<uint16_t> mods;             // [base[n]]
  const uint16_t* mods_ptr() const { return has_mods ? mods.p : nullptr; }
  int64_t count() const { return (int64_t)len.size(); }
};
