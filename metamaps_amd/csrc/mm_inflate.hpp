// BGZF block inflate: the DEFLATE decode core (RFC 1951) and the lane-parallel CRC32, written once for the device kernel (mm_inflate.hip,
// one wavefront per block) and for the host (plain g++: tests/test_inflate_core.cpp checks it against zlib on the CPU).
//
// The core is generic over a lane policy P:
//   P::W                       lanes (64 on the device, 1 on the host)
//   p.lane()                   this lane, 0..W-1
//   p.ballot(b)                bit l set iff lane l passed b (bit 0 = b on the host)
//   p.popc(m), p.popc_below(m) set bits of m, and those of lanes below this one
//   p.sync()                   every lane's LDS writes before it are visible to every lane behind it
//   p.xor_all(v)               XOR of v over the lanes, returned to every lane
//   p.begin_input(in, n)       the deflate range a bit reader is about to read
//   p.ensure(pos)              (uniform) input bytes [pos, pos + 64) can be read with p.in_byte; the device stages them in an LDS ring
//   p.in_byte(in, n, pos)      input byte pos (0 at or past n)
// Symbol decoding is serial and wave-uniform: every lane runs the same bit reader over the same bytes and reaches the same decisions; only the
// table builds, the match copies, the stored-block copies and the CRC run across lanes.
//
// Bounds: every input byte read is clamped to the deflate range of the block (a read past it yields 0 and counts as overrun, which fails the
// block); every output write is checked against ISIZE (the output buffer holds at least ISIZE bytes, and ISIZE <= 65536 is checked first);
// every back-reference is checked against the bytes produced so far.  Whatever the bytes say, a block ends with a status and the core
// touches nothing outside [in, in + in_len) and [out, out + isize).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MMI_HD __host__ __device__ inline
#else
#define MMI_HD inline
#endif
#if defined(__clang__)
#define MMI_UNROLL _Pragma("unroll")
#else
#define MMI_UNROLL
#endif

namespace mmi {

enum Status : int32_t { OK = 0, BAD_STREAM = 1, BAD_LENGTH = 2, BAD_CRC = 3, BAD_HEADER = 4 };
constexpr uint32_t MAX_ISIZE = 65536;
constexpr int FAST_BITS = 10;                                   // primary lookup: codes up to 10 bits in one probe; longer ones walk the counts

// ---- CRC32 (reflected, polynomial 0xEDB88320) ---------------------------------------------------------------------------------------
struct CrcTables { uint32_t byte[256]; uint32_t x2n[32]; };     // byte: one-byte steps; x2n[k] = x^(2^k) mod P (the shift constants)
// the constant tables of a decode: length and distance bases, their extra bits, the code-length code order, the CRC tables
struct Consts {
  CrcTables crc;
  uint16_t lbase[29]; uint8_t lext[29];
  uint16_t dbase[30]; uint8_t dext[30];
  uint8_t clord[19];
};
constexpr uint32_t CRC_POLY = 0xEDB88320u;
MMI_HD constexpr uint32_t crc_multmodp(uint32_t a, uint32_t b) {  // a * b mod P (bit 31 is x^0)
  uint32_t m = 1u << 31, p = 0;
  for (;;) {
    if (a & m) { p ^= b; if ((a & (m - 1)) == 0) break; }
    m >>= 1;
    b = (b & 1) ? (b >> 1) ^ CRC_POLY : b >> 1;
  }
  return p;
}
constexpr CrcTables make_crc_tables() {
  CrcTables t{};
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ CRC_POLY : c >> 1;
    t.byte[i] = c;
  }
  uint32_t p = 1u << 30;                                        // x^1
  for (int k = 0; k < 32; ++k) { t.x2n[k] = p; p = crc_multmodp(p, p); }
  return t;
}
constexpr Consts make_consts() {
  Consts c{};
  c.crc = make_crc_tables();
  for (int i = 0, base = 3; i < 28; ++i) { c.lext[i] = (uint8_t)(i < 8 ? 0 : (i - 4) / 4); c.lbase[i] = (uint16_t)base; base += 1 << c.lext[i]; }
  c.lbase[28] = 258; c.lext[28] = 0;
  for (int i = 0, base = 1; i < 30; ++i) { c.dext[i] = (uint8_t)(i < 4 ? 0 : (i - 2) / 2); c.dbase[i] = (uint16_t)base; base += 1 << c.dext[i]; }
  const uint8_t ord[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  for (int i = 0; i < 19; ++i) c.clord[i] = ord[i];
  return c;
}
// x^(8 n) mod P: what multiplies a CRC register to move it over n zero bytes
MMI_HD uint32_t crc_shift_bytes(const CrcTables& T, uint32_t n) {
  uint32_t p = 1u << 31;
  for (int k = 3; n; n >>= 1, ++k) if (n & 1) p = crc_multmodp(T.x2n[k & 31], p);
  return p;
}

// CRC32 of buf[0, n) (zlib's crc32(0, buf, n)), across the lanes: lane l takes one contiguous piece, its register (started at 0) is shifted
// over the bytes behind the piece, and the pieces are XORed together with the shifted initial register.  Piece lengths are a multiple of 4
// with an odd number of words, so the lanes' byte reads at one step fall into different LDS banks.
template <class P>
MMI_HD uint32_t crc32_lanes(P& p, const CrcTables& T, const uint8_t* buf, uint32_t n) {
  uint32_t piece = (((n + P::W - 1) / P::W) + 3) & ~3u;
  if (P::W > 1 && ((piece >> 2) & 1) == 0) piece += 4;
  const uint32_t lo = p.lane() * piece < n ? p.lane() * piece : n;
  const uint32_t hi = lo + piece < n ? lo + piece : n;
  uint32_t c = 0;
  for (uint32_t i = lo; i < hi; ++i) c = T.byte[(c ^ buf[i]) & 255] ^ (c >> 8);
  uint32_t v = hi > lo ? crc_multmodp(crc_shift_bytes(T, n - hi), c) : 0;
  if (p.lane() == 0) v ^= crc_multmodp(crc_shift_bytes(T, n), 0xFFFFFFFFu);
  return ~p.xor_all(v);
}

// ---- Huffman tables -----------------------------------------------------------------------------------------------------------------
// fast[i]: the symbol and length of the code whose bit-reversed first FAST_BITS bits are i (sym | len << 9), 0 if no code of at most
// FAST_BITS bits starts there (a longer code, or none: the slow walk over cnt/sorted decides).
struct Huff {
  uint16_t fast[1 << FAST_BITS];
  uint16_t cnt[16];                                              // codes per length
  uint16_t sorted[288];                                          // symbols in canonical order
};

// lens[0, n) -> h.  Returns false for an over-subscribed set, or an incomplete one unless it is a single code of length 1 (allowed where
// `single_ok`, as zlib allows it for literal/length and distance codes; an empty set is accepted too and fails on its first decode).
template <class P>
MMI_HD bool build_huff(P& p, Huff& h, const uint8_t* lens, int n, bool single_ok, uint16_t* rank_of) {
  uint32_t cnt[16];
MMI_UNROLL
  for (int l = 0; l < 16; ++l) cnt[l] = 0;
  for (int base = 0; base < n; base += P::W) {                   // rank of each symbol among the symbols of its length: ballots per length
    const int s = base + (int)p.lane();
    const int L = s < n ? lens[s] : 0;
    uint32_t rank = 0;
MMI_UNROLL
    for (int l = 1; l < 16; ++l) {
      const uint64_t m = p.ballot(s < n && L == l);
      if (L == l) rank = cnt[l] + p.popc_below(m);
      cnt[l] += p.popc(m);
    }
    if (s < n) rank_of[s] = (uint16_t)rank;                      // (read back below by the same lane)
  }
  int left = 1, maxl = 0;
MMI_UNROLL
  for (int l = 1; l < 16; ++l) { left = (left << 1) - (int)cnt[l]; if (left < 0) return false; if (cnt[l]) maxl = l; }
  if (left > 0 && maxl > 0 && !(single_ok && maxl == 1)) return false;
  uint32_t offs[16], first[16];
  offs[0] = 0; first[0] = 0;
  uint32_t o = 0, f = 0;
MMI_UNROLL
  for (int l = 1; l < 16; ++l) { f = (f + (l > 1 ? cnt[l - 1] : 0)) << 1; first[l] = f; offs[l] = o; o += cnt[l]; }
  if (p.lane() == 0) {
MMI_UNROLL
    for (int l = 0; l < 16; ++l) h.cnt[l] = (uint16_t)cnt[l];
  }
  for (int base = 0; base < n; base += P::W) {
    const int s = base + (int)p.lane();
    if (s < n) {
      const int L = lens[s];
      uint32_t off = 0;
MMI_UNROLL
      for (int l = 1; l < 16; ++l) if (L == l) off = offs[l];
      if (L) h.sorted[off + rank_of[s]] = (uint16_t)s;
    }
  }
  p.sync();
  for (int i = (int)p.lane(); i < (1 << FAST_BITS); i += P::W) {
    uint32_t r = 0;                                              // the code, MSB first: i bit-reversed
    for (int b = 0; b < FAST_BITS; ++b) r |= ((uint32_t)(i >> b) & 1u) << (FAST_BITS - 1 - b);
    uint16_t e = 0;
MMI_UNROLL
    for (int l = 1; l <= FAST_BITS; ++l) {
      const uint32_t code = r >> (FAST_BITS - l);
      if (!e && code - first[l] < cnt[l]) e = (uint16_t)(h.sorted[offs[l] + code - first[l]] | (l << 9));
    }
    h.fast[i] = e;
  }
  p.sync();
  return true;
}

// ---- bit reader ---------------------------------------------------------------------------------------------------------------------
template <class P>
struct Bits {
  P& p;
  const uint8_t* in; uint32_t len;                               // the deflate range
  uint32_t pos = 0;                                              // next byte to load (may run past len: zeros, counted as overrun)
  uint64_t buf = 0; uint32_t cnt = 0;
  MMI_HD Bits(P& pp, const uint8_t* i, uint32_t n) : p(pp), in(i), len(n) { p.begin_input(i, n); }
  MMI_HD void fill() {
    p.ensure(pos);
    while (cnt <= 56) { const uint64_t b = p.in_byte(in, len, pos); buf |= b << cnt; cnt += 8; ++pos; }
  }
  MMI_HD uint32_t peek(uint32_t n) const { return (uint32_t)(buf & ((1ull << n) - 1)); }
  MMI_HD void drop(uint32_t n) { buf >>= n; cnt -= n; }
  MMI_HD uint32_t take(uint32_t n) { const uint32_t v = peek(n); drop(n); return v; }
  MMI_HD bool overrun() const { return (uint64_t)pos * 8 - cnt > (uint64_t)len * 8; }
  MMI_HD void align() { drop(cnt & 7); }
  MMI_HD uint64_t bitpos() const { return (uint64_t)pos * 8 - cnt; }   // the next bit to be taken
  MMI_HD void seek(uint64_t bit) { pos = (uint32_t)(bit >> 3); buf = 0; cnt = 0; fill(); drop((uint32_t)(bit & 7)); }   // (forward only on the device)
};

// one symbol of h (needs >= 15 bits in the buffer); -1 for a code that is not in the set
template <class B>
MMI_HD int decode_sym(B& b, const Huff& h) {
  const uint16_t e = h.fast[b.peek(FAST_BITS)];
  if (e) { b.drop(e >> 9); return e & 511; }
  int code = 0, first = 0, index = 0;                            // canonical walk, one bit at a time (codes over FAST_BITS bits, or none)
  for (int l = 1; l < 16; ++l) {
    code |= (int)((b.buf >> (l - 1)) & 1);
    const int c = h.cnt[l];
    if (code - c < first) { b.drop((uint32_t)l); return h.sorted[index + (code - first)]; }
    index += c; first += c; first <<= 1; code <<= 1;
  }
  return -1;
}

// ---- the block --------------------------------------------------------------------------------------------------------------------
// LDS (device) / stack (host) scratch of one block's decode
struct Scratch {
  Huff lit, dist;
  uint8_t lens[320];
  uint16_t rank[320];
};

template <class P, class T>
MMI_HD void copy_match(P& p, T* out, uint32_t at, uint32_t dist, uint32_t len) {
  const uint32_t src = at - dist;
  if (dist >= len) { for (uint32_t i = p.lane(); i < len; i += P::W) out[at + i] = out[src + i]; }
  else for (uint32_t i = p.lane(); i < len; i += P::W) out[at + i] = out[src + i % dist];   // overlapping: the period repeats
  p.sync();
}

MMI_HD uint16_t rd16(const uint8_t* q) { return (uint16_t)(q[0] | (q[1] << 8)); }
MMI_HD uint32_t rd32(const uint8_t* q) { return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24); }

// The Huffman tables of a fixed (type 1) or dynamic (type 2) block whose three header bits `b` has just taken: S.lit and S.dist, the dynamic
// header's code lengths read from `b`.  BAD_STREAM for anything RFC 1951 or zlib rejects.  (inflate_raw here and the plain gzip decoder of
// mm_gzip.hpp share it.)
template <class P>
MMI_HD int32_t read_tables(P& p, Scratch& S, const Consts& K, Bits<P>& b, uint32_t type) {
  int nlit = 288, ndist = 32;                                  // (fixed codes: the distance code has 32 symbols, 30 and 31 invalid, as in zlib)
  if (type == 1) {
    for (int s = (int)p.lane(); s < 320; s += P::W) S.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
    p.sync();
  } else {                                                     // dynamic: the code-length code first (built into S.dist)
    nlit = (int)b.take(5) + 257; ndist = (int)b.take(5) + 1;
    const int ncl = (int)b.take(4) + 4;
    if (nlit > 286 || ndist > 30) return BAD_STREAM;
    for (int k = (int)p.lane(); k < 19; k += P::W) S.lens[k] = 0;
    p.sync();
    for (int i = 0; i < ncl; ++i) {
      if (b.cnt < 3) b.fill();
      const uint8_t v = (uint8_t)b.take(3);
      if (p.lane() == 0) S.lens[K.clord[i]] = v;
    }
    p.sync();
    if (b.overrun() || !build_huff(p, S.dist, S.lens, 19, false, S.rank)) return BAD_STREAM;
    const int total = nlit + ndist;
    int i = 0;
    uint8_t prev = 0;
    while (i < total) {
      b.fill();
      if (b.overrun()) return BAD_STREAM;
      const int sym = decode_sym(b, S.dist);
      if (sym < 0) return BAD_STREAM;
      if (sym < 16) { if (p.lane() == 0) S.lens[i] = (uint8_t)sym; prev = (uint8_t)sym; ++i; continue; }
      uint32_t rep; uint8_t v;
      if (sym == 16) { if (i == 0) return BAD_STREAM; v = prev; rep = 3 + b.take(2); }
      else if (sym == 17) { v = 0; rep = 3 + b.take(3); }
      else { v = 0; rep = 11 + b.take(7); }
      if (i + (int)rep > total) return BAD_STREAM;
      for (uint32_t k = p.lane(); k < rep; k += P::W) S.lens[i + k] = v;
      i += (int)rep; prev = v;
    }
    if (b.overrun()) return BAD_STREAM;
    p.sync();
    if (S.lens[256] == 0) return BAD_STREAM;                   // no end-of-block code
  }
  if (!build_huff(p, S.lit, S.lens, nlit, true, S.rank)) return BAD_STREAM;
  if (!build_huff(p, S.dist, S.lens + nlit, ndist, true, S.rank)) return BAD_STREAM;
  return OK;
}

// The deflate stream in[0, n) into out[0, isize): BAD_STREAM for anything RFC 1951 or zlib rejects (and for output beyond isize), BAD_LENGTH
// if the stream ends before isize bytes.  Trailing bytes behind the final block are ignored, as zlib's inflate(Z_FINISH) ignores them.
template <class P>
MMI_HD int32_t inflate_raw(P& p, Scratch& S, const Consts& K, const uint8_t* in, uint32_t n, uint8_t* out, uint32_t isize) {
  Bits<P> b(p, in, n);
  uint32_t o = 0;
  for (bool last = false; !last;) {
    b.fill();
    last = b.take(1);
    const uint32_t type = b.take(2);
    if (type == 0) {                                             // stored
      b.align();
      b.fill();
      const uint32_t len = b.take(16), nlen = b.take(16);
      if (b.overrun() || len != (~nlen & 0xFFFF)) return BAD_STREAM;
      const uint32_t src = b.pos - b.cnt / 8;                    // (what is left in the bit buffer is whole bytes)
      if (src + len > n || o + len > isize) return BAD_STREAM;
      for (uint32_t i = p.lane(); i < len; i += P::W) out[o + i] = in[src + i];
      p.sync();
      o += len;
      b.pos = src + len; b.buf = 0; b.cnt = 0;
      continue;
    }
    if (type == 3) return BAD_STREAM;
    const int32_t ts = read_tables(p, S, K, b, type);
    if (ts != OK) return ts;
    for (;;) {
      b.fill();
      if (b.overrun()) return BAD_STREAM;
      const int sym = decode_sym(b, S.lit);
      if (sym < 0) return BAD_STREAM;
      if (sym < 256) {
        if (o >= isize) return BAD_STREAM;
        if (p.lane() == 0) out[o] = (uint8_t)sym;
        ++o;
        continue;
      }
      if (sym == 256) break;
      if (sym > 285) return BAD_STREAM;
      const uint32_t len = K.lbase[sym - 257] + b.take(K.lext[sym - 257]);
      const int ds = decode_sym(b, S.dist);
      if (ds < 0 || ds > 29) return BAD_STREAM;
      const uint32_t dist = K.dbase[ds] + b.take(K.dext[ds]);
      if (dist > o || o + len > isize) return BAD_STREAM;
      p.sync();                                                  // (lane 0's literals before the copy reads them)
      copy_match(p, out, o, dist, len);
      o += len;
    }
    if (b.overrun()) return BAD_STREAM;
  }
  p.sync();
  return o == isize ? OK : BAD_LENGTH;
}

// One whole BGZF block (gzip member with the BC field) blk[0, blk_len): its header, deflate data, CRC32 and ISIZE.  The inflated bytes go
// to out[0, ISIZE) (out holds MAX_ISIZE bytes); *isize_out gets ISIZE when the header is sound.
template <class P>
MMI_HD int32_t inflate_bgzf(P& p, Scratch& S, const Consts& K, const uint8_t* blk, uint32_t blk_len, uint8_t* out, uint32_t* isize_out) {
  *isize_out = 0;
  if (blk_len < 26) return BAD_HEADER;
  const uint32_t hdr = 12u + rd16(blk + 10);
  if (hdr + 8 > blk_len) return BAD_HEADER;
  const uint32_t crc = rd32(blk + blk_len - 8), isize = rd32(blk + blk_len - 4);
  if (isize > MAX_ISIZE) return BAD_LENGTH;
  *isize_out = isize;
  const int32_t st = inflate_raw(p, S, K, blk + hdr, blk_len - hdr - 8, out, isize);
  if (st != OK) return st;
  return crc32_lanes(p, K.crc, out, isize) == crc ? OK : BAD_CRC;
}

// the host's lane policy: one lane (the CPU tests and any host caller of the core)
struct HostLanes {
  static constexpr uint32_t W = 1;
  uint32_t lane() const { return 0; }
  uint64_t ballot(bool b) const { return b ? 1 : 0; }
  uint32_t popc(uint64_t m) const { return (uint32_t)__builtin_popcountll(m); }
  uint32_t popc_below(uint64_t) const { return 0; }
  void sync() const {}
  uint32_t xor_all(uint32_t v) const { return v; }
  void begin_input(const uint8_t*, uint32_t) const {}
  void ensure(uint32_t) const {}
  uint8_t in_byte(const uint8_t* in, uint32_t n, uint32_t pos) const { return pos < n ? in[pos] : 0; }
};

}  // namespace mmi
