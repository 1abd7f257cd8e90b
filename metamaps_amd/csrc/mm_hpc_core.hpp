// Homopolymer compression (--hpc): the word-level pure functions and the coordinate map's look-up ("Homopolymer
// compression").  hpc(S) replaces every maximal run of equal bytes of S (as hashed: upper-cased ASCII, IUPAC and N kept) by one such byte.
//   keep mask   bit j of a packed word's mask: base j differs from the base before it (that base starts a run and is kept)
//   extraction  the kept 2-bit fields of a word, closed up towards bit 0
//   select      position of the j-th set bit of a 64-bit word
//   raw / rawlast   compressed position -> raw position of the first / last base of its run, from the run-start bitmap (1 bit per raw
//                   stream position) and the sampled select (raw position of every 512th kept base of a contig)
//
// Compiles for host (unit tests: tests/test_hpc_core.cpp via g++, also under ASan/UBSan) and device.
#pragma once
#include <stdint.h>

#ifndef MM_HD
#if defined(__HIPCC__)
#define MM_HD __host__ __device__ inline
#else
#define MM_HD inline
#endif
#endif

namespace mm {

constexpr int HPC_SAMPLE_SHIFT = 9;                              // one select sample per 512 kept bases of a contig

MM_HD int hpc_popc64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(x);
#else
  return __builtin_popcountll(x);
#endif
}

// 16 bases per word, base j at bits [2j, 2j+2).  prev_last: the 2-bit code of the base before base 0 (the previous word's base 15).
// The first base of a sequence and the positions under exception runs are not decided here (the caller forces / rewrites those bits).
MM_HD uint32_t hpc_keep_mask(uint32_t w, uint32_t prev_last) {
  uint32_t x = w ^ ((w << 2) | (prev_last & 3u));
  x = (x | (x >> 1)) & 0x55555555u;                              // bit 2j: field j differs
  x = (x | (x >> 1)) & 0x33333333u;                              // close the even bits up into 16
  x = (x | (x >> 2)) & 0x0f0f0f0fu;
  x = (x | (x >> 4)) & 0x00ff00ffu;
  x = (x | (x >> 8)) & 0x0000ffffu;
  return x;
}

// the fields of w whose bit is set in mask16, in order, from bit 0 up; *count = how many
MM_HD uint32_t hpc_extract(uint32_t w, uint32_t mask16, int* count) {
  mask16 &= 0xffffu;
  if (mask16 == 0xffffu) { *count = 16; return w; }
  uint32_t out = 0; int c = 0;
  while (mask16) {
    const int j = __builtin_ctz(mask16);
    out |= ((w >> (2 * j)) & 3u) << (2 * c);
    ++c;
    mask16 &= mask16 - 1;
  }
  *count = c;
  return out;
}

// position of the j-th (0-based) set bit of x; x has more than j set bits
MM_HD int hpc_select64(uint64_t x, int j) {
  int pos = 0;
  for (int width = 32; width >= 1; width >>= 1) {
    const uint64_t lowmask = (width == 32) ? 0xffffffffull : ((1ull << width) - 1);
    const int c = hpc_popc64((x >> pos) & lowmask);
    if (j >= c) { j -= c; pos += width; }
  }
  return pos;
}

// number of set bits of the bitmap below stream position g, given the exclusive prefix of the per-word popcounts
MM_HD uint64_t hpc_rank(const uint64_t* bitmap, const uint64_t* word_rank, uint64_t g) {
  const uint64_t b = g >> 6; const int s = (int)(g & 63);
  return word_rank[b] + (s ? (uint64_t)hpc_popc64(bitmap[b] & ((1ull << s) - 1)) : 0u);
}

// The map of a set of sequences: bit g of `bitmap` is set iff stream position g (= base[i] + raw position) starts a run; samp[samp_off[i] + s]
// is the raw position of kept base 512 s of sequence i.
struct HpcMapView {
  const uint64_t* bitmap; const uint64_t* base; const int32_t* rawlen; const int32_t* clen; const uint64_t* samp_off; const uint32_t* samp;
  int64_t n;
};

// raw(i, p): raw position of the first base of the run that became compressed base p; rawlen + (p - clen) from the end on (the reference
// reports end = start + len - 1 without clamping, so positions past the contig end translate too); p < 0 is returned as it is
MM_HD int64_t hpc_raw_first(const HpcMapView& M, int64_t i, int64_t p) {
  const int64_t cl = M.clen[i];
  if (p < 0) return p;
  if (p >= cl) return (int64_t)M.rawlen[i] + (p - cl);
  const uint64_t g = M.base[i] + M.samp[M.samp_off[i] + (uint64_t)(p >> HPC_SAMPLE_SHIFT)];
  int64_t need = p & ((1 << HPC_SAMPLE_SHIFT) - 1);            // set bits to pass, from the sample's own bit on
  uint64_t b = g >> 6;
  uint64_t x = M.bitmap[b] & (~0ull << (g & 63));
  for (;;) {
    const int c = hpc_popc64(x);
    if (need < c) return (int64_t)((b << 6) + (uint64_t)hpc_select64(x, (int)need) - M.base[i]);
    need -= c;
    x = M.bitmap[++b];                                           // (p < clen: the bit exists inside the sequence)
  }
}
// rawlast(i, p): raw position of the last base of that run, same rule beyond the end
MM_HD int64_t hpc_raw_last(const HpcMapView& M, int64_t i, int64_t p) {
  const int64_t cl = M.clen[i];
  if (p < 0) return p;
  if (p >= cl) return (int64_t)M.rawlen[i] + (p - cl);
  if (p + 1 < cl) return hpc_raw_first(M, i, p + 1) - 1;
  return (int64_t)M.rawlen[i] - 1;
}

}  // namespace mm
