// The coordinate sort of BAM records and their BAI index (mm_bam_sorter_*; DESIGN.md section 1, "Sorted BAM"; SAM specification section 5.2): the
// definitions, written once for the kernels of mm_bam_sort.hip and for the host (plain g++: tests/test_bam_sort_core.cpp holds them to tests/bai_ref.py).
//
//   order    records ascend by sort_key(ref, pos); equal keys stay in the order they were given (run, then index in the run): a stable sort.
//   stream   the sorted records back to back; out_off[i] is record i's first byte, out_off[n] the stream's length.  The stream is cut into members of
//            MEMBER_RAW inflated bytes, the last one shorter; member m starts at file offset member_at[m], and member_at[n_members] is where the
//            end-of-file block starts.  voff(byte) = member_at[byte / MEMBER_RAW] << 16 | byte % MEMBER_RAW, and member_at[n_members] << 16 for the byte behind
//            the stream's last, which no member holds; a record has vs = voff(out_off[i]) and ve = voff(out_off[i + 1]), the byte after its last.
//   window   output bytes [lo, hi) are made at a time.  Workgroup c of the gather takes the SPAN bytes [lo + c SPAN, ...): upper_record finds the
//            first record that reaches into them, clip gives the part of each record that lies inside, copy_bytes moves it.
//   copy     source and destination have any byte residues.  Equal mod 16: 16-byte loads and stores between a head and a tail of bytes.  Otherwise the
//            destination is walked in aligned 32-bit words, each put together from the one or two aligned source words that hold its bytes.  The
//            aligned source words may start up to 3 bytes before src and end up to 3 bytes behind src + len: the caller's buffer holds them.
//   bins     bin = reg2bin(beg, end), end = pos + max(1, reference span).  Sorted by bin_key(ref, bin) with the ordinal (the place in the file) as the
//            value, stably, a bin's records are neighbours with ordinals ascending; chunk_head marks the first of every run of consecutive ordinals,
//            which is one chunk [vs of its first record, ve of its last].
//   linear   M[i] = the maximum of end_key(ref, end) over the records 0..i (ref ascends along the file, so the maximum never looks back over a
//            reference's first record).  Window w of reference r starts at the vs of the first record i of r with M[i] > end_key(r, w << 14): that
//            is the first record whose end lies behind the window's start; it overlaps window w, or, if it starts behind it, it is the first record
//            of the next window that has one, whose value window w takes.
#pragma once
#include "mm_bam_core.hpp"
#include <vector>

namespace mmbs {

constexpr int64_t MEMBER_RAW = 65280;                             // inflated bytes of every member but the last
constexpr int64_t COORD_END = (int64_t)1 << 29;                   // BAI holds coordinates below this
constexpr uint32_t PSEUDO_BIN = 37450;
constexpr int LINEAR_SHIFT = 14;
constexpr int64_t SPAN = 8192;                                    // output bytes one wavefront gathers

MM_HD uint64_t sort_key(int32_t ref, int32_t pos) { return (uint64_t)(uint32_t)ref << 32 | (uint32_t)pos; }
MM_HD uint64_t end_key(int32_t ref, int32_t end) { return (uint64_t)(uint32_t)ref << 32 | (uint32_t)end; }
MM_HD uint64_t bin_key(int32_t ref, uint32_t bin) { return (uint64_t)(uint32_t)ref << 16 | bin; }
MM_HD int64_t n_members(int64_t stream_bytes) { return (stream_bytes + MEMBER_RAW - 1) / MEMBER_RAW; }
MM_HD uint64_t voff(int64_t byte, const int64_t* member_at, int64_t stream_bytes) {   // (the byte behind the stream's last: the end-of-file block's first)
  return byte == stream_bytes ? (uint64_t)member_at[n_members(stream_bytes)] << 16 : (uint64_t)member_at[byte / MEMBER_RAW] << 16 | (uint64_t)(byte % MEMBER_RAW);
}
MM_HD int32_t n_intervals(int32_t max_end) { return max_end > 0 ? 1 + ((max_end - 1) >> LINEAR_SHIFT) : 0; }

// the first i in [a, b) with v[i] > t; b if there is none (v never falls)
template <class T> MM_HD int64_t first_above(const T* v, int64_t a, int64_t b, T t) {
  while (a < b) { const int64_t mid = a + (b - a) / 2; if (v[mid] > t) b = mid; else a = mid + 1; }
  return a;
}
// the first record that has a byte behind `byte`: the first i in [0, n) with out_off[i + 1] > byte
MM_HD int64_t upper_record(const int64_t* out_off, int64_t n, int64_t byte) { return first_above<int64_t>(out_off + 1, 0, n, byte); }

// the part of a record (stream bytes [o, o + size), source bytes from src_off on) inside [lo, hi): where it comes from, where it goes (from lo), its length
struct Piece { int64_t src, dst, len; };
MM_HD Piece clip(int64_t o, int64_t size, int64_t src_off, int64_t lo, int64_t hi) {
  const int64_t a = o > lo ? o : lo, b = o + size < hi ? o + size : hi;
  Piece p; p.src = src_off + (a - o); p.dst = a - lo; p.len = b > a ? b - a : 0;
  return p;
}

// element j of the records sorted by (bin_key, ordinal) starts a chunk
MM_HD bool chunk_head(const uint64_t* key, const int64_t* ord, int64_t j) { return j == 0 || key[j] != key[j - 1] || ord[j] != ord[j - 1] + 1; }

struct alignas(16) V16 { uint32_t x, y, z, w; };
// len bytes from src to dst by the lanes of p (P::W, p.lane() as in mm_bam_core.hpp); the buffers do not overlap
template <class P> MM_HD void copy_bytes(P& p, const uint8_t* src, uint8_t* dst, int64_t len) {
  const int64_t l = (int64_t)p.lane();
  if ((((uintptr_t)src ^ (uintptr_t)dst) & 15) == 0) {
    const int64_t pre = (int64_t)((16 - ((uintptr_t)dst & 15)) & 15), head = pre < len ? pre : len, nvec = (len - head) >> 4;
    for (int64_t i = l; i < head; i += P::W) dst[i] = src[i];
    const V16* vs = (const V16*)(src + head);
    V16* vd = (V16*)(dst + head);
    for (int64_t i = l; i < nvec; i += P::W) vd[i] = vs[i];
    for (int64_t i = head + (nvec << 4) + l; i < len; i += P::W) dst[i] = src[i];
    return;
  }
  const int64_t pre = (int64_t)((4 - ((uintptr_t)dst & 3)) & 3), head = pre < len ? pre : len, nw = (len - head) >> 2;
  for (int64_t i = l; i < head; i += P::W) dst[i] = src[i];
  const uint32_t r = (uint32_t)((uintptr_t)(src + head) & 3);
  const uint32_t* sa = (const uint32_t*)(src + head - r);
  uint32_t* da = (uint32_t*)(dst + head);
  if (r == 0) for (int64_t i = l; i < nw; i += P::W) da[i] = sa[i];
  else for (int64_t i = l; i < nw; i += P::W) da[i] = sa[i] >> (8 * r) | sa[i + 1] << (32 - 8 * r);
  for (int64_t i = head + (nw << 2) + l; i < len; i += P::W) dst[i] = src[i];
}

// The host's part of the index: the bytes of the .bai from what the device made.  ref_start[r] .. ref_start[r + 1]: the records of reference r in file
// order; vs / ve per record; the chunks ascending by (key, first ordinal) with key = bin_key(ref, bin); win_off[r] .. win_off[r + 1]: the windows of r in ioff.
struct BaiParts {
  int32_t n_ref; const int64_t* ref_start; const uint64_t* first_vs; const uint64_t* last_ve;   // (first_vs / last_ve per reference; unread where it has no record)
  int64_t n_chunks; const uint64_t* chunk_key; const uint64_t* chunk_vs; const uint64_t* chunk_ve;
  const int64_t* win_off; const uint64_t* ioff;
};
inline void put_le(std::vector<uint8_t>& o, uint64_t v, int bytes) { for (int k = 0; k < bytes; ++k) o.push_back((uint8_t)(v >> (8 * k))); }
inline std::vector<uint8_t> bai_bytes(const BaiParts& p) {
  std::vector<uint8_t> o = {'B', 'A', 'I', 1};
  put_le(o, (uint32_t)p.n_ref, 4);
  int64_t c = 0;
  for (int32_t r = 0; r < p.n_ref; ++r) {
    const int64_t n_rec = p.ref_start[r + 1] - p.ref_start[r];
    int64_t c1 = c, bins = 0;
    for (; c1 < p.n_chunks && (int64_t)(p.chunk_key[c1] >> 16) == r; ++c1) bins += c1 == c || p.chunk_key[c1] != p.chunk_key[c1 - 1];
    put_le(o, (uint32_t)(n_rec ? bins + 1 : 0), 4);
    while (c < c1) {
      int64_t e = c;
      while (e < c1 && p.chunk_key[e] == p.chunk_key[c]) ++e;
      put_le(o, p.chunk_key[c] & 0xFFFF, 4); put_le(o, (uint32_t)(e - c), 4);
      for (; c < e; ++c) { put_le(o, p.chunk_vs[c], 8); put_le(o, p.chunk_ve[c], 8); }
    }
    if (n_rec) { put_le(o, PSEUDO_BIN, 4); put_le(o, 2, 4); put_le(o, p.first_vs[r], 8); put_le(o, p.last_ve[r], 8); put_le(o, (uint64_t)n_rec, 8); put_le(o, 0, 8); }
    put_le(o, (uint32_t)(p.win_off[r + 1] - p.win_off[r]), 4);
    for (int64_t w = p.win_off[r]; w < p.win_off[r + 1]; ++w) put_le(o, p.ioff[w], 8);
  }
  put_le(o, 0, 8);                                                 // n_no_coor
  return o;
}

}  // namespace mmbs
