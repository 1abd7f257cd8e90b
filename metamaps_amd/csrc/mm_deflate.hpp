// BGZF block deflate: the encoder core (RFC 1951 / 1952, the BGZF container of the SAM specification), written once for the device kernel
// (mm_deflate.hip, one wavefront per BGZF block) and for the host (plain g++: tests/test_deflate_core.cpp checks it against zlib on the CPU).
// The CRC32 is the lane-parallel one of mm_inflate.hpp.
//
// One call turns up to 65 280 input bytes into one complete BGZF member: 18 header bytes with the BC subfield and BSIZE, ONE DEFLATE block
// (dynamic Huffman codes, or stored where that is not larger), CRC32, ISIZE.  The bytes are a pure function of the input: every step below is
// defined over groups of G = 64 positions whatever the number of lanes, so the host (one lane, which walks each group in a loop) and the
// device (64 lanes) write the same member.
//
//   search   in steps of 64 positions, one per lane: hash the four bytes at the position, read the head table AS THE PREVIOUS STEPS LEFT
//            IT (a match never starts inside the step's own 64 bytes; it may run into them), measure the match (4..258 bytes, at most
//            32 768 back), then insert the 64 positions (the highest position wins a slot).  The greedy parse of the step is a walk over
//            the 64 match lengths from where the last token ended; the tokens go to a buffer of 4 bytes per token (global memory on the
//            device), the two histograms are counted with LDS atomics.
//   codes    code lengths from the histograms: a rank sort of the used symbols across the lanes, the two-queue Huffman merge and the
//            length limit (15 / 7 bits: counts per length moved down until Kraft's sum is 1, longest codes to the rarest symbols) on lane 0.
//            A code with fewer than two used symbols gets a second one, as zlib does, so every code set is complete.
//   size     the block's exact bit count from the histograms, before a bit is written: BSIZE goes into the header, and a block that would
//            not be smaller than its stored form is written stored.
//   emit     64 tokens a round: each lane's code and extra bits (at most 48), a prefix sum of the bit counts over the lanes, an OR into a
//            4 KiB window of 32-bit words in LDS, which goes out to the member in 16-byte pieces when it fills.
//
// A lane policy P (the host's below, the device's in mm_deflate.hip) has:
//   P::W, p.lane(), p.sync()    as in mm_inflate.hpp
//   p.xor_all(v)                for crc32_lanes
//   p.insert_max(slot, v)       *slot = max(*slot, v) over the lanes that call it, visible after the next sync
//   p.add(a, v), p.or32(a, v)   *a += v, *a |= v: lanes may hit the same word
//   p.scan_excl(v, &total)      the sum of v over the lanes below this one, and over all lanes (host: 0 and v: its lanes run one by one)
// Per-lane code is written as `for (l = p.lane(); l < 64; l += P::W)`: once per lane on the device, a loop over the group on the host.
// Values that cross a sync live in the scratch, never in a lane's variables.
//
// Bounds: the input lies in S.in[0, n) with n <= 65 280 and zeros behind it; a match candidate comes out of the head table, which only
// ever holds positions below the one being searched; the token buffer holds n + 1 entries and a step adds at most one per position; the
// member is at most n + 31 bytes and `dst` holds MEMBER_MAX.
#pragma once
#include "mm_inflate.hpp"
#include <cstddef>

namespace mmd {

using mmi::Consts;
constexpr uint32_t BLOCK_IN = 0xff00;                            // input bytes per BGZF block (what bgzip uses)
constexpr uint32_t MEMBER_MAX = 65536;                           // bytes a member's destination holds (a member is at most BLOCK_IN + 31)
constexpr int64_t LAUNCH_BLOCKS = 4096;                          // blocks per launch of the kernel (255 MiB of input)
constexpr uint32_t G = 64;                                       // positions per search step, tokens per emit round
constexpr uint32_t HASH_BITS = 12, MIN_MATCH = 4, MAX_MATCH = 258, WINDOW = 32768;
constexpr uint32_t STAGE_WORDS = 1024, STAGE_MARGIN = 112;       // the output window; a round adds at most 64 * 48 bits = 96 words
constexpr uint32_t TOK_CAP = BLOCK_IN + 1;                       // tokens of a block (one per position at most) + the end-of-block
constexpr uint32_t TOK_EOB = 0x40000000u, TOK_MATCH = 0x80000000u;   // token: a literal's byte, or TOK_MATCH | dist - 1 << 8 | len - 3
constexpr uint32_t NLIT = 286, NDIST = 30, NCL = 19;

struct alignas(16) V4 { uint32_t x[4]; };

// scratch of the code construction (dead during the search and the emit)
struct Build {
  uint32_t freq[2 * 288];                                        // leaves in rising order, then the merged nodes
  uint16_t parent[2 * 288];
  uint16_t sorted[288];                                          // used symbols by (frequency, symbol)
  uint8_t depth[2 * 288];
  uint32_t cnt[16], nc[16];                                      // codes per length, the next code of each length
};
struct Scratch {
  alignas(16) uint8_t in[BLOCK_IN + 16];                         // the block, zeros behind it
  union alignas(16) {
    uint16_t head[1u << HASH_BITS];                              // search: position + 1 of the last insert per hash (0: none)
    Build build;                                                 // codes
    uint32_t stage[STAGE_WORDS];                                 // emit: the window of output words
  } u;
  uint32_t lhist[288], dhist[32], clhist[NCL];
  uint16_t lcode[288], dcode[32], clcode[NCL];                   // codes, bit-reversed (DEFLATE packs them from the most significant bit)
  uint8_t lens[320];                                             // literal/length code lengths, the distance code's behind them
  uint8_t cllen[NCL];
  uint8_t clsym[320], clext[320];                                // the code lengths run-length coded: symbol 0..18 and its extra bits' value
  uint16_t mlen[G], mdist[G], hsh[G];                            // a search step's matches (0: none) and hashes (0xffff: nothing to insert)
  uint32_t tail[4];
  uint32_t n_items, hlit, hdist, hclen, bits, pad[2];
};

// the bit writer: uniform state; the words live in S.u.stage
struct Writer {
  uint8_t* dst;                                                  // the member (16-byte aligned)
  uint32_t wbase = 0;                                            // stage[0] is word wbase of the member
  uint32_t bitpos = 0;                                           // next bit of the member
};

MMI_HD uint32_t ld32(const uint8_t* in, uint32_t pos) {          // the four bytes at pos, from aligned words
  const uint8_t* q = (const uint8_t*)__builtin_assume_aligned(in + (pos & ~3u), 4);
  uint32_t w0, w1;
  __builtin_memcpy(&w0, q, 4);
  __builtin_memcpy(&w1, q + 4, 4);
  return (uint32_t)(((uint64_t)w0 | ((uint64_t)w1 << 32)) >> ((pos & 3) * 8));
}
MMI_HD uint32_t hash4(uint32_t w) { return (w * 2654435761u) >> (32 - HASH_BITS); }
MMI_HD uint32_t clz32(uint32_t v) { return (uint32_t)__builtin_clz(v); }
MMI_HD uint32_t ctz32(uint32_t v) { return (uint32_t)__builtin_ctz(v); }
MMI_HD uint32_t rev_bits(uint32_t c, uint32_t len) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < len; ++i) r |= ((c >> i) & 1u) << (len - 1 - i);
  return r;
}
// length 3..258 -> index of its code (0..28), extra bits and their value
MMI_HD void len_code(uint32_t len, uint32_t& code, uint32_t& eb, uint32_t& ev) {
  const uint32_t l = len - 3;
  if (l < 8) { code = l; eb = 0; ev = 0; return; }
  if (l == 255) { code = 28; eb = 0; ev = 0; return; }
  eb = 29 - clz32(l);                                            // (floor(log2 l) - 2)
  code = 4 * eb + 4 + ((l >> eb) & 3);
  ev = l & ((1u << eb) - 1);
}
MMI_HD void dist_code(uint32_t dist, uint32_t& code, uint32_t& eb, uint32_t& ev) {
  const uint32_t t = dist - 1;
  if (t < 4) { code = t; eb = 0; ev = 0; return; }
  const uint32_t hb = 31 - clz32(t);
  eb = hb - 1;
  code = 2 * hb + ((t >> eb) & 1);
  ev = t & ((1u << eb) - 1);
}
MMI_HD uint32_t lcode_ext(uint32_t c) { return c < 8 || c == 28 ? 0 : (c - 4) / 4; }   // extra bits of length code c, distance code c
MMI_HD uint32_t dcode_ext(uint32_t c) { return c < 4 ? 0 : (c - 2) / 2; }

// ---- output -------------------------------------------------------------------------------------------------------------------------
// `nbits` (<= 48) bits of `bits` behind the lanes' below; every lane of a round calls it once (nbits 0: nothing)
template <class P>
MMI_HD void put(P& p, Scratch& S, Writer& w, uint64_t bits, uint32_t nbits) {
  uint32_t total;
  const uint32_t at = w.bitpos + p.scan_excl(nbits, &total);
  if (nbits) {
    const uint32_t i = (at >> 5) - w.wbase, sh = at & 31;
    const uint64_t rest = sh ? bits >> (32 - sh) : bits >> 32;
    p.or32(&S.u.stage[i], (uint32_t)(bits << sh));
    if ((uint32_t)rest) p.or32(&S.u.stage[i + 1], (uint32_t)rest);
    if ((uint32_t)(rest >> 32)) p.or32(&S.u.stage[i + 2], (uint32_t)(rest >> 32));
  }
  w.bitpos += total;
}
// whole 16-byte pieces of the window out to the member; `all`: everything up to the last bit (the member is done)
template <class P>
MMI_HD void flush(P& p, Scratch& S, Writer& w, bool all) {
  const uint32_t have = ((w.bitpos + 31) >> 5) - w.wbase;        // words with bits in them
  if (!all && have < STAGE_WORDS - STAGE_MARGIN) return;
  p.sync();
  const uint32_t full = (w.bitpos >> 5) - w.wbase;               // words no later bit goes into
  const uint32_t k = all ? (have + 3) & ~3u : full & ~3u;
  V4* const d = (V4*)(w.dst + (std::size_t)w.wbase * 4);
  const V4* const s = (const V4*)S.u.stage;
  for (uint32_t i = p.lane(); i < k / 4; i += P::W) d[i] = s[i];
  if (all) return;
  for (uint32_t i = p.lane(); i < 4; i += P::W) S.tail[i] = S.u.stage[k + i];
  p.sync();
  for (uint32_t i = p.lane(); i < STAGE_WORDS; i += P::W) S.u.stage[i] = 0;
  p.sync();
  for (uint32_t i = p.lane(); i < 4; i += P::W) S.u.stage[i] = S.tail[i];
  p.sync();
  w.wbase += k;
}

// ---- code construction ------------------------------------------------------------------------------------------------------------
// hist[0, n) -> lens[0, n) (0 for unused symbols, at most maxbits) and the bit-reversed canonical codes.  Fewer than two used symbols: one
// or two of symbols 0 / 1 are counted once for the construction (S.pad says which; the histogram itself is left as it was).
template <class P>
MMI_HD void build_code(P& p, Scratch& S, uint32_t* hist, uint32_t n, uint32_t maxbits, uint8_t* lens, uint16_t* codes) {
  Build& B = S.u.build;
  if (p.lane() == 0) {
    uint32_t used = 0;
    for (uint32_t s = 0; s < n; ++s) used += hist[s] != 0;
    S.pad[0] = S.pad[1] = 0xffffffffu;
    for (uint32_t k = 0; used < 2; ++k, ++used) { const uint32_t s = hist[0] == 0 ? 0 : 1; hist[s] = 1; S.pad[k] = s; }
    S.n_items = used;
  }
  p.sync();
  const uint32_t u = S.n_items;
  for (uint32_t s = p.lane(); s < n; s += P::W) {                // rank sort by (frequency, symbol)
    lens[s] = 0;
    const uint32_t f = hist[s];
    if (!f) continue;
    uint32_t rank = 0;
    for (uint32_t j = 0; j < n; ++j) { const uint32_t g = hist[j]; rank += g && (g < f || (g == f && j < s)); }
    B.sorted[rank] = (uint16_t)s;
    B.freq[rank] = f;
  }
  p.sync();
  if (p.lane() == 0) {
    // two queues: leaves [0, u) in rising order, merged nodes [u, 2u - 1) come out in rising order too
    uint32_t a = 0, b = u, next = u;
    for (; next < 2 * u - 1; ++next) {
      const uint32_t p0 = a < u && (b >= next || B.freq[a] <= B.freq[b]) ? a++ : b++;
      const uint32_t p1 = a < u && (b >= next || B.freq[a] <= B.freq[b]) ? a++ : b++;
      B.freq[next] = B.freq[p0] + B.freq[p1];
      B.parent[p0] = B.parent[p1] = (uint16_t)next;
    }
    uint32_t* const cnt = B.cnt;
    uint32_t* const nc = B.nc;
    for (int l = 0; l < 16; ++l) cnt[l] = 0;
    B.depth[2 * u - 2] = 0;
    for (uint32_t i = 2 * u - 2; i-- > 0;) {
      const uint32_t d = B.depth[B.parent[i]] + 1u;
      B.depth[i] = (uint8_t)(d < 255 ? d : 255);
      if (i < u) ++cnt[d < maxbits ? d : maxbits];
    }
    // the length limit: move counts down until Kraft's sum is 1 again
    uint32_t total = 0;
    for (uint32_t l = 1; l <= maxbits; ++l) total += cnt[l] << (maxbits - l);
    while (total > (1u << maxbits)) {
      --cnt[maxbits];
      for (uint32_t l = maxbits - 1; l > 0; --l) if (cnt[l]) { --cnt[l]; cnt[l + 1] += 2; break; }
      --total;
    }
    uint32_t i = 0;                                              // the rarest symbols take the longest codes
    for (uint32_t l = maxbits; l > 0; --l) for (uint32_t c = 0; c < cnt[l]; ++c) lens[B.sorted[i++]] = (uint8_t)l;
    uint32_t code = 0;
    cnt[0] = 0;
    for (uint32_t l = 1; l <= maxbits; ++l) { code = (code + cnt[l - 1]) << 1; nc[l] = code; }
    for (uint32_t s = 0; s < n; ++s) { const uint32_t l = lens[s]; codes[s] = l ? (uint16_t)rev_bits(nc[l]++, l) : 0; }
    for (int k = 0; k < 2; ++k) if (S.pad[k] != 0xffffffffu) hist[S.pad[k]] = 0;
  }
  p.sync();
}

// ---- one member ---------------------------------------------------------------------------------------------------------------------
template <class P>
MMI_HD void put_header(P& p, Scratch& S, Writer& w, uint32_t member) {
  for (uint32_t l = p.lane(); l < G; l += P::W) {
    // 1f 8b 08 04, no time, XFL 0, OS 255, XLEN 6, 'B' 'C', 2, BSIZE
    const uint64_t b = l < 8 ? 0x0000000004088b1full >> (8 * l) : l < 16 ? 0x000243420006ff00ull >> (8 * (l - 8)) : (uint64_t)(member - 1) >> (8 * (l & 1));
    put(p, S, w, l < 18 ? b & 255 : 0, l < 18 ? 8 : 0);
  }
}
template <class P>
MMI_HD void put_trailer(P& p, Scratch& S, Writer& w, uint32_t crc, uint32_t n) {
  w.bitpos = (w.bitpos + 7) & ~7u;
  for (uint32_t l = p.lane(); l < G; l += P::W) put(p, S, w, l < 4 ? (crc >> (8 * l)) & 255 : l < 8 ? (n >> (8 * (l - 4))) & 255 : 0, l < 8 ? 8 : 0);
}

// S.in[0, n) (zeros in S.in[n, n + 16)), 1 <= n <= BLOCK_IN  ->  one BGZF member at dst (16-byte aligned, MEMBER_MAX bytes); tok holds
// TOK_CAP tokens.  Returns the member's bytes; *stored_out says whether it fell back to a stored block.
template <class P>
MMI_HD uint32_t deflate_member(P& p, Scratch& S, const Consts& K, uint32_t n, uint32_t* tok, uint8_t* dst, uint32_t* stored_out) {
  const uint32_t crc = mmi::crc32_lanes(p, K.crc, S.in, n);
  for (uint32_t i = p.lane(); i < (1u << HASH_BITS); i += P::W) S.u.head[i] = 0;
  for (uint32_t i = p.lane(); i < 288; i += P::W) S.lhist[i] = 0;
  for (uint32_t i = p.lane(); i < 32; i += P::W) S.dhist[i] = 0;
  for (uint32_t i = p.lane(); i < NCL; i += P::W) S.clhist[i] = 0;
  p.sync();

  // ---- search and parse
  uint32_t ntok = 0, next = 0;
  for (uint32_t base = 0; base < n; base += G) {
    for (uint32_t l = p.lane(); l < G; l += P::W) {
      const uint32_t pos = base + l;
      uint32_t len = 0, dist = 0, h = 0xffff;
      if (pos + MIN_MATCH <= n) {
        const uint32_t first = ld32(S.in, pos);
        h = hash4(first);
        const uint32_t c = S.u.head[h];
        if (c && pos - (c - 1) <= WINDOW && ld32(S.in, c - 1) == first) {
          const uint32_t cand = c - 1, maxlen = n - pos < MAX_MATCH ? n - pos : MAX_MATCH;
          uint32_t i = 4;
          while (i < maxlen) {
            const uint32_t x = ld32(S.in, pos + i) ^ ld32(S.in, cand + i);
            if (x) { i += ctz32(x) >> 3; break; }
            i += 4;
          }
          len = i < maxlen ? i : maxlen;
          dist = pos - cand;
        }
      }
      S.mlen[l] = (uint16_t)len; S.mdist[l] = (uint16_t)(dist - (dist != 0)); S.hsh[l] = (uint16_t)h;
    }
    p.sync();
    for (uint32_t l = p.lane(); l < G; l += P::W) {
      const uint32_t h = S.hsh[l];
      if (h != 0xffff) p.insert_max(&S.u.head[h], base + l + 1);
      else p.insert_max(nullptr, 0);
    }
    // the greedy parse of the step: the positions a token starts at (every lane walks the same lengths)
    const uint32_t cnt = n - base < G ? n - base : G;
    uint64_t starts = 0;
    uint32_t q = next - base;
    while (q < cnt) { starts |= 1ull << q; const uint32_t L = S.mlen[q]; q += L ? L : 1; }
    next = base + q;
    for (uint32_t l = p.lane(); l < G; l += P::W) {
      if (!((starts >> l) & 1)) continue;
      const uint32_t at = ntok + (uint32_t)__builtin_popcountll(starts & ((1ull << l) - 1));
      const uint32_t len = S.mlen[l];
      if (len) {
        const uint32_t d1 = S.mdist[l];
        tok[at] = TOK_MATCH | (d1 << 8) | (len - 3);
        uint32_t c, eb, ev;
        len_code(len, c, eb, ev); p.add(&S.lhist[257 + c], 1);
        dist_code(d1 + 1, c, eb, ev); p.add(&S.dhist[c], 1);
      } else {
        const uint32_t b = S.in[base + l];
        tok[at] = b;
        p.add(&S.lhist[b], 1);
      }
    }
    ntok += (uint32_t)__builtin_popcountll(starts);
    p.sync();
  }
  if (p.lane() == 0) { tok[ntok] = TOK_EOB; S.lhist[256] = 1; }
  ++ntok;
  p.sync();

  // ---- codes
  build_code(p, S, S.lhist, NLIT, 15, S.lens, S.lcode);
  if (p.lane() == 0) {
    uint32_t hl = NLIT; while (hl > 257 && S.lens[hl - 1] == 0) --hl;
    S.hlit = hl;
  }
  p.sync();
  const uint32_t hlit = S.hlit;
  build_code(p, S, S.dhist, NDIST, 15, S.lens + hlit, S.dcode);
  if (p.lane() == 0) {
    uint32_t hd = NDIST; while (hd > 1 && S.lens[hlit + hd - 1] == 0) --hd;
    S.hdist = hd;
    // the code lengths, run-length coded (RFC 1951 3.2.7): 16 repeats the previous length 3..6 times, 17 / 18 are runs of zeros
    const uint32_t total = hlit + hd;
    uint32_t m = 0;
    for (uint32_t i = 0; i < total;) {
      const uint32_t v = S.lens[i];
      uint32_t run = 1;
      while (i + run < total && S.lens[i + run] == v) ++run;
      i += run;
      if (v == 0) {
        while (run >= 11) { const uint32_t r = run < 138 ? run : 138; S.clsym[m] = 18; S.clext[m++] = (uint8_t)(r - 11); run -= r; }
        if (run >= 3) { S.clsym[m] = 17; S.clext[m++] = (uint8_t)(run - 3); run = 0; }
      } else {
        S.clsym[m] = (uint8_t)v; S.clext[m++] = 0; --run;
        while (run >= 3) { const uint32_t r = run < 6 ? run : 6; S.clsym[m] = 16; S.clext[m++] = (uint8_t)(r - 3); run -= r; }
      }
      for (; run; --run) { S.clsym[m] = (uint8_t)v; S.clext[m++] = 0; }
    }
    for (uint32_t i = 0; i < m; ++i) ++S.clhist[S.clsym[i]];
    S.bits = 0;
  }
  p.sync();
  const uint32_t hdist = S.hdist;
  build_code(p, S, S.clhist, NCL, 7, S.cllen, S.clcode);         // (n_items is build_code's scratch: the item count is recounted below)
  if (p.lane() == 0) {
    uint32_t hc = NCL; while (hc > 4 && S.cllen[K.clord[hc - 1]] == 0) --hc;
    S.hclen = hc;
    uint32_t m = 0;
    for (uint32_t s = 0; s < NCL; ++s) m += S.clhist[s];
    S.n_items = m;
  }
  p.sync();
  const uint32_t hclen = S.hclen, n_items = S.n_items;

  // ---- size: the block's bits, exactly
  for (uint32_t s = p.lane(); s < 288 + 32 + NCL; s += P::W) {
    uint32_t b = 0;
    if (s < 288) { if (s < NLIT) b = S.lhist[s] * (S.lens[s] + (s > 256 ? lcode_ext(s - 257) : 0)); }
    else if (s < 320) { const uint32_t d = s - 288; if (d < hdist) b = S.dhist[d] * (S.lens[hlit + d] + dcode_ext(d)); }
    else { const uint32_t c = s - 320; b = S.clhist[c] * (S.cllen[c] + (c == 16 ? 2 : c == 17 ? 3 : c == 18 ? 7 : 0)); }
    if (b) p.add(&S.bits, b);
  }
  p.sync();
  const uint32_t bits = 3 + 14 + 3 * hclen + S.bits;
  const uint32_t dyn_bytes = (bits + 7) >> 3, stored_bytes = n + 5;
  const bool stored = dyn_bytes >= stored_bytes;
  *stored_out = stored;
  const uint32_t member = 18 + (stored ? stored_bytes : dyn_bytes) + 8;
  p.sync();                                                      // (the code construction's scratch becomes the output window)
  for (uint32_t i = p.lane(); i < STAGE_WORDS; i += P::W) S.u.stage[i] = 0;
  p.sync();

  // ---- emit
  Writer w;
  w.dst = dst;
  put_header(p, S, w, member);
  if (stored) {
    for (uint32_t l = p.lane(); l < G; l += P::W) {
      const uint64_t h = 1ull | ((uint64_t)n << 8) | ((uint64_t)(~n & 0xffff) << 24);   // final stored block, LEN, NLEN
      put(p, S, w, l < 5 ? (h >> (8 * l)) & 255 : 0, l < 5 ? 8 : 0);
    }
    for (uint32_t base = 0; base < n; base += G) {
      for (uint32_t l = p.lane(); l < G; l += P::W) put(p, S, w, base + l < n ? S.in[base + l] : 0, base + l < n ? 8 : 0);
      flush(p, S, w, false);
    }
  } else {
    for (uint32_t l = p.lane(); l < G; l += P::W) {
      uint64_t v = 0; uint32_t nb = 0;
      if (l == 0) { v = 5u | ((hlit - 257) << 3) | ((hdist - 1) << 8) | ((hclen - 4) << 13); nb = 17; }
      else if (l - 1 < hclen) { v = S.cllen[K.clord[l - 1]]; nb = 3; }
      put(p, S, w, v, nb);
    }
    for (uint32_t base = 0; base < n_items; base += G) {
      for (uint32_t l = p.lane(); l < G; l += P::W) {
        uint64_t v = 0; uint32_t nb = 0;
        if (base + l < n_items) {
          const uint32_t c = S.clsym[base + l];
          nb = S.cllen[c];
          v = S.clcode[c] | ((uint64_t)S.clext[base + l] << nb);
          nb += c == 16 ? 2 : c == 17 ? 3 : c == 18 ? 7 : 0;
        }
        put(p, S, w, v, nb);
      }
      flush(p, S, w, false);
    }
    for (uint32_t base = 0; base < ntok; base += G) {
      for (uint32_t l = p.lane(); l < G; l += P::W) {
        uint64_t v = 0; uint32_t nb = 0;
        if (base + l < ntok) {
          const uint32_t t = tok[base + l];
          if (t & TOK_MATCH) {
            uint32_t c, eb, ev;
            len_code((t & 255) + 3, c, eb, ev);
            nb = S.lens[257 + c]; v = S.lcode[257 + c] | ((uint64_t)ev << nb); nb += eb;
            dist_code(((t >> 8) & 0x7fff) + 1, c, eb, ev);
            const uint32_t dl = S.lens[hlit + c];
            v |= (uint64_t)(S.dcode[c] | (ev << dl)) << nb; nb += dl + eb;
          } else {
            const uint32_t s = t == TOK_EOB ? 256 : t;
            v = S.lcode[s]; nb = S.lens[s];
          }
        }
        put(p, S, w, v, nb);
      }
      flush(p, S, w, false);
    }
  }
  put_trailer(p, S, w, crc, n);
  flush(p, S, w, true);
  p.sync();
  return member;
}

MMI_HD int64_t n_blocks_of(int64_t in_bytes) { return (in_bytes + BLOCK_IN - 1) / BLOCK_IN; }
MMI_HD int64_t bound(int64_t in_bytes) { return in_bytes + 31 * n_blocks_of(in_bytes); }

// the host's lane policy: one lane
struct HostLanes {
  static constexpr uint32_t W = 1;
  uint32_t lane() const { return 0; }
  void sync() const {}
  uint32_t xor_all(uint32_t v) const { return v; }
  void insert_max(uint16_t* slot, uint32_t v) const { if (slot && *slot < v) *slot = (uint16_t)v; }
  void add(uint32_t* a, uint32_t v) const { *a += v; }
  void or32(uint32_t* a, uint32_t v) const { *a |= v; }
  uint32_t scan_excl(uint32_t v, uint32_t* total) const { *total = v; return 0; }
};

}  // namespace mmd
