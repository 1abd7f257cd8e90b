// Plain gzip (RFC 1952, one DEFLATE stream per member, no block index) inflated in parallel by speculative decoding, the technique of pugz
// (Kerbiriou & Chikhi, 2019) and rapidgzip (Knespel & Brunst, 2023).  One source for the device (mm_gzip.hip: one wavefront per chunk) and for
// the host (plain g++, one lane: tests/test_gzip_core.cpp checks it against zlib on the CPU).  The RFC 1951 pieces — bit reader, Huffman
// tables, symbol decode, match copy — are mm_inflate.hpp's; the lane policy P is the one described there.
//
// The compressed stream is cut into chunks of C bytes.  Chunk 0 of a round starts where the stream is known to be.  Every later chunk
//   - finds the first bit offset at or after its nominal start that plausibly begins a DEFLATE block (gz_find: a dynamic header whose
//     counts are in range and whose code-length code is complete, or a stored header with LEN == ~NLEN on a byte boundary, then a trial
//     decode of TRIAL symbols' output whose literals are all text — queries and references are FASTA/FASTQ);
//   - decodes from there with an unknown 32 KiB window (gz_decode): the window entries are *markers* 256 + i, and a back-reference into the
//     window copies the marker, so markers propagate through later copies.  The decode stops at the first block boundary at or after the
//     next chunk's nominal start, at the end of a final block, or suspends (output full, input short) between two symbols.
// The driver (Stream) then walks the chunks in order: chunk k's speculation is accepted only if the decode before it stopped exactly at
// chunk k's start bit; otherwise the chunk is decoded again from where its predecessor stopped, with the known window.  A bad candidate
// costs time, never correctness: a stream in which nothing is found (only fixed-Huffman blocks, binary data) decodes, sequentially.
// Each accepted piece overwrites its window region with the real window (bytes, or INVALID before the member start), so one lookup
// resolves any marker of the piece; the window carried to the next piece is the resolved last 32 KiB.  After the walk one parallel pass
// resolves every piece into bytes and its CRC32, and the driver checks every member's CRC32 and ISIZE.
//
// Bounds: a decode reads only in[0, n) (bytes past n read as 0 and fail the decode as overrun) and writes only w[WIN, WIN + cap) of its slot;
// a back-reference reaches at most 32 768 entries back, which the window region in front of the output holds.
#pragma once
#include "mm_inflate.hpp"

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace mmg {

using mmi::Bits;
using mmi::Consts;
using mmi::Scratch;

constexpr uint32_t WIN = 32768;                                  // the DEFLATE window, in entries, in front of every slot's output
constexpr uint16_t INVALID = 0xFFFF;                             // a window entry before the member start (a reference to it is corrupt data)
constexpr uint64_t NONE = ~0ull;
constexpr uint64_t DEFAULT_CHUNK = (uint64_t)1 << 18;                  // compressed bytes per chunk (MM_GZIP_CHUNK_BYTES)
constexpr uint32_t TRIAL = 4096;                                 // output entries a finder's trial decode must produce without a fault
constexpr uint32_t IN_MARGIN = 1024;                             // with more input to come, a decode suspends this close to the end of `in`

enum Status : int32_t { OK = 0, BAD_STREAM = 1, NOT_FOUND = 5, NOT_TEXT = 6 };
enum How : uint32_t { BOUNDARY = 0, FINAL = 1, FULL = 2, SHORT = 3 };   // stopped at a block boundary >= stop, after a final block, out of room, out of input
enum Flags : uint32_t { F_MORE = 1, F_TEXT = 2, F_FIND = 4 };   // more input follows `in`; literals must be text; find the start in [lo, hi)

struct Job { uint64_t start, hdr, stop, lo, hi; uint32_t flags, slot; };
// start: where the decode began (the candidate for F_FIND); end: where it stopped; hdr: the header bit of the block it stopped inside (NONE
// at a block boundary); len: output entries
struct Res { uint64_t start, end, hdr; uint32_t len, how; int32_t status, pad; };

MMI_HD bool is_text(uint32_t c) { return (c >= 32 && c < 127) || c == 10 || c == 13 || c == 9; }

// Decode from bit `start` (a block header, or — hdr != NONE — a symbol boundary inside the Huffman block whose header is at `hdr`) into
// w[WIN, WIN + cap), the window being w[0, WIN).
template <class P>
MMI_HD void gz_decode(P& p, Scratch& S, const Consts& K, const uint8_t* in, uint32_t n, uint16_t* w, uint32_t cap, uint64_t start,
                      uint64_t hdr, uint64_t stop, uint32_t flags, Res& r) {
  Bits<P> b(p, in, n);
  uint16_t* const out = w + WIN;
  uint32_t o = 0;
  bool last = false, in_block = false;
  uint64_t h = NONE;
  r.start = start; r.hdr = NONE; r.how = BOUNDARY; r.status = OK; r.pad = 0;
#define MMG_END(st, how_, at, hb) do { r.status = (st); r.how = (how_); r.end = (at); r.hdr = (hb); r.len = o; p.sync(); return; } while (0)
  if (hdr != NONE) {
    b.seek(hdr);
    last = b.take(1);
    const uint32_t type = b.take(2);
    if (type != 1 && type != 2) MMG_END(BAD_STREAM, BOUNDARY, hdr, NONE);
    if (read_tables(p, S, K, b, type) != mmi::OK || b.overrun()) MMG_END(BAD_STREAM, BOUNDARY, hdr, NONE);
    b.seek(start);
    h = hdr; in_block = true;
  } else {
    b.seek(start);
  }
  for (;;) {
    if (!in_block) {
      const uint64_t at = b.bitpos();
      if (at >= stop) MMG_END(OK, BOUNDARY, at, NONE);
      if ((flags & F_MORE) && (at >> 3) + IN_MARGIN > n) MMG_END(OK, SHORT, at, NONE);
      b.fill();
      last = b.take(1);
      const uint32_t type = b.take(2);
      h = at;
      if (type == 0) {                                           // stored: whole, or not at all (a suspension comes back to its header)
        b.align();
        b.fill();
        const uint32_t len = b.take(16), nlen = b.take(16);
        if (b.overrun() || len != (~nlen & 0xFFFF)) MMG_END(BAD_STREAM, BOUNDARY, at, NONE);
        const uint32_t src = b.pos - b.cnt / 8;
        if ((uint64_t)src + len > n) { if (flags & F_MORE) MMG_END(OK, SHORT, at, NONE); MMG_END(BAD_STREAM, BOUNDARY, at, NONE); }
        if (o + len > cap) MMG_END(OK, FULL, at, NONE);
        bool bad = false;
        for (uint32_t i = p.lane(); i < len; i += P::W) { const uint8_t c = in[src + i]; out[o + i] = c; bad |= (flags & F_TEXT) && !is_text(c); }
        if (p.ballot(bad)) MMG_END(NOT_TEXT, BOUNDARY, at, NONE);
        p.sync();
        o += len;
        b.pos = src + len; b.buf = 0; b.cnt = 0;
        if (last) MMG_END(OK, FINAL, (uint64_t)(src + len) * 8, NONE);
        continue;
      }
      if (type == 3) MMG_END(BAD_STREAM, BOUNDARY, at, NONE);
      if (read_tables(p, S, K, b, type) != mmi::OK) MMG_END(BAD_STREAM, BOUNDARY, at, NONE);
      in_block = true;
    }
    for (;;) {
      const uint64_t s0 = b.bitpos();
      if ((flags & F_MORE) && (s0 >> 3) + IN_MARGIN > n) MMG_END(OK, SHORT, s0, h);
      b.fill();
      if (b.overrun()) MMG_END(BAD_STREAM, BOUNDARY, s0, NONE);
      const int sym = decode_sym(b, S.lit);
      if (sym < 0) MMG_END(BAD_STREAM, BOUNDARY, s0, NONE);
      if (sym < 256) {
        if (o >= cap) MMG_END(OK, FULL, s0, h);
        if ((flags & F_TEXT) && !is_text((uint32_t)sym)) MMG_END(NOT_TEXT, BOUNDARY, s0, NONE);
        if (p.lane() == 0) out[o] = (uint16_t)sym;
        ++o;
        continue;
      }
      if (sym == 256) break;
      if (sym > 285) MMG_END(BAD_STREAM, BOUNDARY, s0, NONE);
      const uint32_t len = K.lbase[sym - 257] + b.take(K.lext[sym - 257]);
      const int ds = decode_sym(b, S.dist);
      if (ds < 0 || ds > 29) MMG_END(BAD_STREAM, BOUNDARY, s0, NONE);
      const uint32_t dist = K.dbase[ds] + b.take(K.dext[ds]);
      if (b.overrun()) MMG_END(BAD_STREAM, BOUNDARY, s0, NONE);
      if (o + len > cap) MMG_END(OK, FULL, s0, h);
      p.sync();                                                  // (lane 0's literals before the copy reads them)
      mmi::copy_match(p, w, WIN + o, dist, len);                 // (dist <= 32768: the window in front of the output covers it)
      o += len;
    }
    in_block = false;
    if (b.overrun()) MMG_END(BAD_STREAM, BOUNDARY, b.bitpos(), NONE);
    if (last) MMG_END(OK, FINAL, b.bitpos(), NONE);
  }
#undef MMG_END
}

// the 57 bits of in[] from bit `bit` on (bytes past n read as 0)
MMI_HD uint64_t bits57(const uint8_t* in, uint32_t n, uint64_t bit) {
  const uint64_t q = bit >> 3;
  uint64_t v = 0;
  for (uint32_t i = 0; i < 8; ++i) v |= (uint64_t)(q + i < n ? in[q + i] : 0) << (8 * i);
  return v >> (bit & 7);
}
// the finder's cheap test of one bit offset (one lane each): a dynamic header with HLIT <= 29, HDIST <= 29 and a complete code-length code,
// or a stored header (zero padding to the byte boundary, LEN == ~NLEN).  Fixed-Huffman blocks are not looked for: too many false positives.
MMI_HD bool plausible(const uint8_t* in, uint32_t n, uint64_t h) {
  const uint64_t v = bits57(in, n, h);
  const uint32_t type = (uint32_t)(v >> 1) & 3;
  if (type == 2) {
    if (((v >> 3) & 31) > 29 || ((v >> 8) & 31) > 29) return false;
    const uint32_t ncl = (uint32_t)((v >> 13) & 15) + 4;
    const uint64_t c = bits57(in, n, h + 17);
    uint32_t kraft = 0;                                          // in units of 2^-7
    for (uint32_t i = 0; i < ncl; ++i) { const uint32_t l = (uint32_t)(c >> (3 * i)) & 7; if (l) kraft += 128u >> l; }
    return kraft == 128;
  }
  if (type == 0) {
    const uint64_t a = (h + 3 + 7) >> 3;                         // the byte of LEN
    if (a + 4 > n) return false;
    const uint32_t pad = (uint32_t)(a * 8 - (h + 3));
    if ((v >> 3) & ((1u << pad) - 1)) return false;
    const uint32_t len = in[a] | (in[a + 1] << 8), nlen = in[a + 2] | (in[a + 3] << 8);
    return len == (~nlen & 0xFFFFu);
  }
  return false;
}

// First bit in [lo, hi) that passes `plausible` and a trial decode (into the slot's output, which the real decode overwrites); NONE if none.
template <class P>
MMI_HD uint64_t gz_find(P& p, Scratch& S, const Consts& K, const uint8_t* in, uint32_t n, uint16_t* w, uint64_t lo, uint64_t hi, uint32_t flags) {
  for (uint64_t base = lo; base < hi; base += P::W) {
    const uint64_t h = base + p.lane();
    uint64_t m = p.ballot(h < hi && plausible(in, n, h));
    while (m) {
      const uint32_t l = (uint32_t)__builtin_ctzll(m);
      m &= m - 1;
      Res t;
      gz_decode(p, S, K, in, n, w, TRIAL, base + l, NONE, NONE, flags, t);
      if (t.status == OK) return base + l;
    }
  }
  return NONE;
}

// One job: a speculative chunk (F_FIND: marker window, find, decode) or a decode from a known position with the window already in place.
template <class P>
MMI_HD void gz_run_job(P& p, Scratch& S, const Consts& K, const uint8_t* in, uint32_t n, uint16_t* w, uint32_t cap, const Job& j, Res& r) {
  if (!(j.flags & F_FIND)) { gz_decode(p, S, K, in, n, w, cap, j.start, j.hdr, j.stop, j.flags, r); return; }
  for (uint32_t i = p.lane(); i < WIN; i += P::W) w[i] = (uint16_t)(256 + i);
  p.sync();
  // a candidate that passed the trial but whose decode fails later (a non-text literal, an invalid code) was a false positive: the search
  // goes on behind it, so one such candidate does not cost the chunk its speculation
  for (uint64_t lo = j.lo;;) {
    const uint64_t start = gz_find(p, S, K, in, n, w, lo, j.hi, j.flags);
    if (start == NONE) { r.start = r.end = r.hdr = NONE; r.len = 0; r.how = BOUNDARY; r.status = NOT_FOUND; r.pad = 0; return; }
    gz_decode(p, S, K, in, n, w, cap, start, NONE, j.stop, j.flags, r);
    if (r.status == OK) return;
    lo = start + 1;
  }
}

// the resolved entry i of a slot whose window region holds the real window (bytes or INVALID): a marker is looked up there once
MMI_HD uint16_t resolve_entry(const uint16_t* w, uint32_t i) {
  const uint16_t v = w[i];
  return v < 256 || v == INVALID ? v : w[v - 256];
}

// ---- the host driver (host code only) ------------------------------------------------------------------------------------------------------------------
// A backend B runs jobs and the window and resolve steps where the slots live (the host below, the device in mm_gzip.hip):
//   b.begin_round(in, n, nslots, cap)        the round's input, and nslots slots of WIN + cap entries
//   b.run(jobs, nj, res)                     the jobs, each on its slot, results back on the host
//   b.win_reset()                            the carried window := INVALID (a member starts)
//   b.win_to_slot(s)                         slot s's window region := the carried window
//   b.win_from_slot(s, len)                  the carried window := the resolved last WIN entries of slot s's [0, WIN + len)
//   b.resolve(pieces, np, dst, crc, bad)     each piece's len entries as bytes to dst (back to back), its CRC32, and the index of its first
//                                            entry that resolves to INVALID (-1: none)
struct Piece { uint32_t slot, len; };

struct Stats {
  int64_t chunks = 0, accepted = 0, redone = 0, skipped = 0;     // chunks = accepted + redone + skipped (covered by the chunk before)
  double t_spec = 0, t_chain = 0, t_resolve = 0, t_total = 0;    // seconds: speculative kernel, sequential walk (with redos), resolve + CRC
};

inline uint32_t crc32_host(const Consts& K, uint32_t crc, const uint8_t* q, size_t n) {
  crc = ~crc;
  for (size_t i = 0; i < n; ++i) crc = K.crc.byte[(crc ^ q[i]) & 255] ^ (crc >> 8);
  return ~crc;
}

// inflated bytes, grown without zero-filling (a segment's output is hundreds of MB, written once by the resolve)
class Bytes {
  std::unique_ptr<uint8_t[]> p_; size_t n_ = 0, cap_ = 0;
 public:
  uint8_t* data() { return p_.get(); }
  size_t size() const { return n_; }
  bool empty() const { return n_ == 0; }
  void clear() { n_ = 0; }
  void truncate(size_t n) { if (n < n_) n_ = n; }
  uint8_t* grow(size_t k) {                                      // k more bytes at the end, uninitialised
    if (n_ + k > cap_) {
      const size_t c = std::max(n_ + k, cap_ + cap_ / 2);
      std::unique_ptr<uint8_t[]> q(new uint8_t[c]);
      if (n_) memcpy(q.get(), p_.get(), n_);
      p_ = std::move(q); cap_ = c;
    }
    n_ += k;
    return p_.get() + n_ - k;
  }
};

template <class B>
class Stream {
 public:
  static constexpr uint64_t DEFAULT_SEGMENT = (uint64_t)128 << 20, MAX_SEGMENT = (uint64_t)1 << 30;
  // the slots of one round (WIN + cap entries per chunk) stay within this many bytes: a small chunk size makes rounds shorter, not larger
  static constexpr uint64_t SLOT_BUDGET = (uint64_t)9 << 29;    // 4.5 GiB
  Stream(B& be, uint64_t chunk, uint64_t segment)
      : be_(be), C_(std::max<uint64_t>(chunk, 256)), SEG_(std::min<uint64_t>(std::max<uint64_t>(segment, 1024), MAX_SEGMENT)) {}
  // n more compressed bytes; last: they end the stream.  0 ok, -1 corrupt data (error(), error_offset()).  Output accumulates in out().
  // The bytes are taken a segment at a time, so the buffered input stays below two segments and a margin whatever n is (positions in it
  // are 32-bit).
  int feed(const uint8_t* q, size_t n, bool last) {
    if (failed_) return -1;
    if (done_) return 0;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = 0;
    size_t at = 0;
    do {
      const size_t k = std::min<size_t>(n - at, (size_t)SEG_);
      buf_.insert(buf_.end(), q + at, q + at + k);
      at += k;
      rc = process(last && at == n);
    } while (rc == 0 && at < n);
    if (last && !failed_) done_ = true;
    st.t_total += secs(t0);
    return rc;
  }
  Bytes& out() { return out_; }
  const std::string& error() const { return err_; }
  uint64_t error_offset() const { return err_off_; }
  uint64_t members() const { return members_; }
  Stats st;

 private:
  // rounds over what is buffered: while a segment and a margin are ahead of the position, or to the end when `last`
  int process(bool last) {
    int rc = 0;
    for (;;) {
      if (phase_ == END) { base_ += buf_.size(); buf_.clear(); break; }
      if (!last && buf_.size() < (pos_ >> 3) + SEG_ + MARGIN) break;
      const bool progress = round(last);
      if (failed_) { rc = -1; break; }
      if (!progress) {
        if (!last) break;
        if (phase_ == HDR && (pos_ >> 3) >= buf_.size()) { phase_ = END; continue; }
        rc = fail(base_ + buf_.size(), "the stream ends inside a gzip member (truncated file)");
        break;
      }
    }
    return rc;
  }
  enum Phase { HDR, DEFL, TRL, END };
  static constexpr uint64_t MARGIN = 4096;
  static constexpr uint32_t HDR_NEED = 1, HDR_BAD = 2, HDR_GARBAGE = 3;
  B& be_;
  const uint64_t C_, SEG_;
  std::vector<uint8_t> buf_;                                     // compressed bytes [base_, base_ + size)
  Bytes out_;
  uint64_t base_ = 0, pos_ = 0, hdr_ = NONE;                     // pos_/hdr_: bits in buf_
  Phase phase_ = HDR;
  bool failed_ = false, done_ = false;
  std::string err_; uint64_t err_off_ = 0;
  uint64_t members_ = 0;
  uint32_t crc_ = 0; uint32_t isize_ = 0;                        // the member so far (flushed pieces)
  std::vector<Piece> pieces_; std::vector<uint64_t> piece_at_;   // pending pieces, and the compressed offset each began at
  const Consts K_ = mmi::make_consts();

  static double secs(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
  int fail(uint64_t off, const std::string& what) {
    if (!failed_) { failed_ = true; err_off_ = off; err_ = what + " at compressed byte offset " + std::to_string(off); }
    return -1;
  }
  // the gzip header at buf_[pos_ / 8): its length, or HDR_* (need more bytes, corrupt, not a header behind a member: trailing garbage)
  uint32_t header(bool last, size_t* hlen) {
    const uint8_t* q = buf_.data() + (pos_ >> 3);
    const size_t a = buf_.size() - (pos_ >> 3);
    const bool first = members_ == 0;
    if (a < 2) return last ? (first && a ? HDR_BAD : HDR_GARBAGE) : HDR_NEED;
    if (q[0] != 0x1f || q[1] != 0x8b) return first ? HDR_BAD : HDR_GARBAGE;
    const uint32_t short_ = last ? HDR_BAD : HDR_NEED;
    if (a < 10) return short_;
    if (q[2] != 8 || (q[3] & 0xE0)) return HDR_BAD;
    size_t i = 10;
    if (q[3] & 4) { if (a < i + 2) return short_; i += 2 + (size_t)(q[i] | (q[i + 1] << 8)); if (a < i) return short_; }
    for (int f = 8; f <= 16; f <<= 1) if (q[3] & f) { const void* z = memchr(q + i, 0, a - i); if (!z) return short_; i = (size_t)((const uint8_t*)z - q) + 1; }
    if (q[3] & 2) {
      if (a < i + 2) return short_;
      if ((crc32_host(K_, 0, q, i) & 0xFFFF) != (uint32_t)(q[i] | (q[i + 1] << 8))) return HDR_BAD;
      i += 2;
    }
    *hlen = i;
    return 0;
  }
  // resolve the pending pieces into out_ and fold their CRCs into the member's
  bool flush() {
    if (pieces_.empty()) return true;
    const auto t0 = std::chrono::steady_clock::now();
    size_t total = 0;
    for (auto& pc : pieces_) total += pc.len;
    const size_t at = out_.size();
    uint8_t* const dst = out_.grow(total);
    std::vector<uint32_t> crc(pieces_.size());
    std::vector<int64_t> bad(pieces_.size());
    be_.resolve(pieces_.data(), (uint32_t)pieces_.size(), dst, crc.data(), bad.data());
    for (size_t i = 0; i < pieces_.size(); ++i) {
      if (bad[i] >= 0) { out_.truncate(at); fail(piece_at_[i], "a back-reference reaches before the start of its gzip member"); return false; }
      crc_ = mmi::crc_multmodp(mmi::crc_shift_bytes(K_.crc, pieces_[i].len), crc_) ^ crc[i];
    }
    pieces_.clear(); piece_at_.clear();
    st.t_resolve += secs(t0);
    return true;
  }
  // the member trailer at the byte behind pos_ (phase TRL): CRC32 and ISIZE checked, then phase HDR.  1 done, 0 more input needed, -1 failed
  int trailer(bool last) {
    if (!flush()) return -1;
    const uint64_t n = buf_.size(), t = (pos_ + 7) >> 3;
    if (t + 8 > n) {
      if (!last) return 0;
      fail(base_ + n, "the stream ends inside a gzip trailer (truncated file)");
      return -1;
    }
    const uint32_t crc = mmi::rd32(buf_.data() + t), isz = mmi::rd32(buf_.data() + t + 4);
    if (crc != crc_) { fail(base_ + t, "gzip member CRC32 mismatch"); return -1; }
    if (isz != isize_) { fail(base_ + t + 4, "gzip member length (ISIZE) mismatch"); return -1; }
    ++members_;
    pos_ = (t + 8) * 8; hdr_ = NONE; phase_ = HDR;
    return 1;
  }
  // one round: at most a segment of chunks from pos_ on.  false if it made no progress.
  bool round(bool last) {
    const uint64_t pos0 = pos_, base0 = base_;
    const Phase ph0 = phase_;
    const uint32_t n = (uint32_t)buf_.size();
    if (phase_ == TRL && trailer(last) <= 0) return after_round(ph0, pos0, base0);   // (a trailer the last round's input ended inside)
    if (phase_ == HDR && !next_member(last)) return after_round(ph0, pos0, base0);
    if (phase_ != DEFL) return after_round(ph0, pos0, base0);
    const uint64_t p0 = pos_ >> 3;
    const uint32_t cap = (uint32_t)std::max<uint64_t>(16 * C_, 66 * 1024);
    const uint64_t kmax = std::max<uint64_t>(1, SLOT_BUDGET / (2 * ((uint64_t)WIN + cap)) - 1);
    const uint64_t R = std::min<uint64_t>(last ? n : n - MARGIN, p0 + std::min<uint64_t>(SEG_, kmax * C_));
    const uint64_t stopR = R >= n ? NONE : R * 8;
    const uint32_t K = (uint32_t)std::max<uint64_t>(1, (R > p0 ? R - p0 + C_ - 1 : 0) / C_);
    auto N = [&](uint32_t k) -> uint64_t { return k == 0 ? pos_ : k >= K ? stopR : (p0 + (uint64_t)k * C_) * 8; };
    const uint32_t more = last ? 0 : F_MORE, REDO = K;
    std::vector<Job> jobs(K);
    std::vector<Res> res(K);
    for (uint32_t k = 0; k < K; ++k) {
      if (k == 0) jobs[k] = Job{pos_, hdr_, N(1), 0, 0, more, 0};
      else jobs[k] = Job{NONE, NONE, N(k + 1), N(k), std::min<uint64_t>(N(k + 1), (uint64_t)n * 8), more | F_TEXT | F_FIND, k};
    }
    const uint64_t hdr0 = hdr_;
    auto t0 = std::chrono::steady_clock::now();
    be_.begin_round(buf_.data(), n, K + 1, cap);
    be_.win_to_slot(0);
    be_.run(jobs.data(), K, res.data());
    st.t_spec += secs(t0);
    t0 = std::chrono::steady_clock::now();
    std::vector<uint8_t> used(K, 0), counted(K, 0);
    int64_t acc = 0, redo = 0;
    bool redo_pending = false, short_ = false;
    auto take = [&](uint32_t slot, const Res& r) {
      if (r.len) {
        pieces_.push_back(Piece{slot, r.len}); piece_at_.push_back(base_ + (r.start >> 3));
        be_.win_from_slot(slot, r.len);
        isize_ += r.len;
      }
      pos_ = r.end;
      hdr_ = (r.how == FULL || r.how == SHORT) ? r.hdr : NONE;
      if (r.how == FINAL) phase_ = TRL;
      short_ = r.how == SHORT;
    };
    for (;;) {
      if (phase_ == TRL) {
        const int t = trailer(last);
        if (t < 0) return true;
        if (t == 0) break;
      }
      if (phase_ == HDR) { if (!next_member(last) || phase_ != DEFL) break; }
      if (hdr_ == NONE && stopR != NONE && pos_ >= stopR) break;
      if (stopR == NONE && pos_ >= (uint64_t)n * 8 && hdr_ == NONE) { fail(base_ + n, "the stream ends inside a gzip member (truncated file)"); return true; }
      uint32_t k = 0;
      if (pos_ >= N(1)) k = (uint32_t)std::min<uint64_t>(K - 1, ((pos_ >> 3) - p0) / C_);
      const Res& s = res[k];
      const bool ok = !used[k] && s.status == OK && s.start == pos_ && (k == 0 ? hdr_ == hdr0 : hdr_ == NONE);
      if (ok) {
        used[k] = 1;
        if (!counted[k]) { counted[k] = 1; ++acc; }
        if (k) be_.win_to_slot(k);
        take(k, s);
      } else {
        if (redo_pending && !flush()) return true;
        Job j{pos_, hdr_, N(k + 1), 0, 0, more, REDO};
        Res r;
        be_.win_to_slot(REDO);
        be_.run(&j, 1, &r);
        if (r.status != OK) { fail(base_ + (r.end >> 3), "corrupt deflate data"); return true; }
        if (!counted[k]) { counted[k] = 1; ++redo; }
        redo_pending = r.len > 0;
        take(REDO, r);
      }
      if (short_) break;                                         // suspended for input: the next round goes on from there
    }
    st.t_chain += secs(t0);
    if (!flush()) return true;
    st.chunks += K; st.accepted += acc; st.redone += redo; st.skipped += K - acc - redo;
    return after_round(ph0, pos0, base0);
  }
  // parse the next member's header at pos_ (phase HDR): DEFL on success, END for trailing garbage; false if more input is needed (or bad)
  bool next_member(bool last) {
    size_t hl = 0;
    const uint32_t h = header(last, &hl);
    if (h == HDR_NEED) return false;
    if (h == HDR_GARBAGE) { phase_ = END; return true; }
    if (h == HDR_BAD) { fail(base_ + (pos_ >> 3), "malformed gzip header"); return false; }
    pos_ += (uint64_t)hl * 8; hdr_ = NONE; phase_ = DEFL; crc_ = 0; isize_ = 0;
    be_.win_reset();
    return true;
  }
  // drop the input behind what a resumed decode still reads; progress = the position or phase moved
  bool after_round(Phase ph0, uint64_t pos0, uint64_t base0) {
    if (failed_) return true;
    uint64_t keep = phase_ == END ? buf_.size() : ((phase_ == DEFL && hdr_ != NONE ? hdr_ : pos_) >> 3);
    keep = std::min<uint64_t>(keep, buf_.size());
    if (keep) {
      buf_.erase(buf_.begin(), buf_.begin() + (std::ptrdiff_t)keep);
      base_ += keep; pos_ -= keep * 8;
      if (hdr_ != NONE) hdr_ -= keep * 8;
    }
    return base_ * 8 + pos_ != base0 * 8 + pos0 || phase_ != ph0;
  }
};

// the host backend: the slots in host memory, the jobs one after the other on one lane
struct HostBackend {
  mmi::HostLanes lanes;
  const Consts K = mmi::make_consts();
  Scratch S;
  const uint8_t* in = nullptr; uint32_t n = 0, cap = 0;
  std::vector<uint16_t> slots, W = std::vector<uint16_t>(WIN, INVALID);
  uint16_t* slot(uint32_t s) { return slots.data() + (size_t)s * (WIN + cap); }
  void begin_round(const uint8_t* i, uint32_t nn, uint32_t nslots, uint32_t c) { in = i; n = nn; cap = c; slots.assign((size_t)nslots * (WIN + cap), 0); }
  void run(const Job* jobs, uint32_t nj, Res* res) { for (uint32_t j = 0; j < nj; ++j) gz_run_job(lanes, S, K, in, n, slot(jobs[j].slot), cap, jobs[j], res[j]); }
  void win_reset() { std::fill(W.begin(), W.end(), INVALID); }
  void win_to_slot(uint32_t s) { std::copy(W.begin(), W.end(), slot(s)); }
  void win_from_slot(uint32_t s, uint32_t len) { const uint16_t* w = slot(s); for (uint32_t t = 0; t < WIN; ++t) W[t] = resolve_entry(w, len + t); }
  void resolve(const Piece* pc, uint32_t np, uint8_t* dst, uint32_t* crc, int64_t* bad) {
    for (uint32_t i = 0; i < np; ++i) {
      const uint16_t* w = slot(pc[i].slot);
      bad[i] = -1;
      for (uint32_t e = 0; e < pc[i].len; ++e) {
        const uint16_t v = resolve_entry(w, WIN + e);
        if (v == INVALID && bad[i] < 0) bad[i] = e;
        dst[e] = (uint8_t)v;
      }
      crc[i] = crc32_host(K, 0, dst, pc[i].len);
      dst += pc[i].len;
    }
  }
};

}  // namespace mmg
