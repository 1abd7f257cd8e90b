// Methylation per sequence motif (mapDirectly --mod-motifs; DESIGN.md section 1, "Modification motifs"), written once for the kernels of mm_motif.hip and for the
// host (plain g++: tests/test_motif_core.cpp holds it to tests/motif_ref.py).
//
//   letters      A = 1, C = 2, G = 4, T = 8, the IUPAC letters their unions, N = 15 (letter_mask; 0 for any other byte).  A reference byte b, as the packed
//                set holds it, has the nibble base_nibble(b): its one bit for A C G T, 0 for every other byte (the set's exception runs) and beyond a contig's
//                ends.  b fits a motif letter x iff nibble(b) & mask(x) != 0: a byte outside A C G T fits nothing, not even N.
//   motif        1 to 32 letters M[0, L) and the offset o of the modified base, M[o] one of A C G T.  f holds mask(M[i]) in nibble i, r the masks of the
//                reverse complement, comp_mask(mask(M[L - 1 - i])) in nibble i; both are 128 bits in two words, nibble i at bits [4i, 4i + 4).
//   window       the nibbles of ref[c][s, s + L) in the same layout.  Every nibble has at most one bit, so the window fits an orientation iff
//                popcount(window & mask) == L (fits).
//   occurrence   + at modified position q: s = q - o >= 0, s + L <= n and the window at s fits f; - at q: s = q - (L - 1 - o) >= 0, s + L <= n and the
//                window at s fits r (occurs).  Never across a contig's end; overlapping occurrences all count.
//   counts       of an occurrence (c, q, strand, j) and every asked code k whose base is M[o]: mmd::segment_rows' at the site (c, q, strand) of the merged
//                table, all zero where the table has no entry.  N_valid = N_mod + N_canonical + N_other; covered iff N_valid >= the minimal coverage,
//                modified iff covered and (double)N_mod >= F * (double)N_valid (covered, modified: the form of mmp::site_kept).
//   combined     a motif equal to its own reverse complement (f == r): the + occurrence at s (site q = s + o) and the - occurrence of the same window (site
//                q' = s + L - 1 - o != q) are one unit at (c, q) whose counts are the sums of both sites.  OWNER: the thread (or loop step) of the + site
//                when the table has an entry of (c, q, +), whatever its classes; else that of the - site (c, q', -).  A unit without either has no row.
//   scan         a tile is SCAN_TILE consecutive stream positions from a multiple of SCAN_TILE; a window that starts in it reaches at most HALO positions
//                beyond it.
#pragma once
#include "mm_mods_core.hpp"

namespace mmt {

constexpr int MAX_MOTIFS = 8, MAX_LEN = 32, HALO = MAX_LEN - 1;
constexpr int SCAN_THREADS = 256, SCAN_PER_THREAD = 8, SCAN_TILE = SCAN_THREADS * SCAN_PER_THREAD;   // 8 nibbles: one 32-bit word of the staged tile per thread
constexpr int SUMS = 5;                                            // per (contig, motif, code): sites, covered, modified, N_valid_cov, N_mod
constexpr double DEFAULT_MIN_FRAC = 0.5;                           // a declared default

MM_HD uint32_t letter_mask(uint8_t x) {
  switch (x) {
    case 'A': return 1; case 'C': return 2; case 'G': return 4; case 'T': return 8;
    case 'R': return 5; case 'Y': return 10; case 'S': return 6; case 'W': return 9; case 'K': return 12; case 'M': return 3;
    case 'B': return 14; case 'D': return 13; case 'H': return 11; case 'V': return 7; case 'N': return 15;
    default: return 0;
  }
}
MM_HD uint32_t base_nibble(uint8_t b) { return b == 'A' ? 1u : b == 'C' ? 2u : b == 'G' ? 4u : b == 'T' ? 8u : 0u; }
MM_HD uint32_t comp_mask(uint32_t m) { return (m & 1u) << 3 | (m & 2u) << 1 | (m & 4u) >> 1 | (m & 8u) >> 3; }   // A <-> T, C <-> G
MM_HD uint8_t mask_base(uint32_t m) { return m == 1 ? 'A' : m == 2 ? 'C' : m == 4 ? 'G' : m == 8 ? 'T' : 0; }   // the letter of a one-bit mask, else 0

struct Motif { uint64_t f[2], r[2]; int32_t len, pos; uint8_t base; };   // base: the letter M[o]
struct Motifs { int32_t n; Motif m[MAX_MOTIFS]; };

// the motif of the 4-bit letter sets mask[0, len) with the modified base at pos; false (and *out untouched) unless len is 1..32, every mask 1..15 and
// mask[pos] has one bit
MM_HD bool make_motif(const uint8_t* mask, int32_t len, int32_t pos, Motif* out) {
  if (len < 1 || len > MAX_LEN || pos < 0 || pos >= len) return false;
  Motif m{{0, 0}, {0, 0}, len, pos, 0};
  for (int32_t i = 0; i < len; ++i) {
    if (mask[i] < 1 || mask[i] > 15) return false;
    m.f[i >> 4] |= (uint64_t)mask[i] << (4 * (i & 15));
    m.r[i >> 4] |= (uint64_t)comp_mask(mask[len - 1 - i]) << (4 * (i & 15));
  }
  m.base = mask_base(mask[pos]);
  if (!m.base) return false;
  *out = m;
  return true;
}
MM_HD bool own_reverse_complement(const Motif& m) { return m.f[0] == m.r[0] && m.f[1] == m.r[1]; }

MM_HD bool fits(uint64_t w0, uint64_t w1, const uint64_t* mask, int32_t len) {
  return (int32_t)(mmd::popc(w0 & mask[0]) + mmd::popc(w1 & mask[1])) == len;
}
// R gives ref.byte(i), contig byte i of 0 .. n - 1 (upper case, as the packed set holds it)
template <class R> MM_HD bool occurs(const R& ref, int64_t n, int64_t q, bool minus, const Motif& m) {
  const int64_t s = q - (minus ? m.len - 1 - m.pos : m.pos);
  if (s < 0 || s + m.len > n) return false;
  uint64_t w[2] = {0, 0};
  for (int32_t i = 0; i < m.len; ++i) w[i >> 4] |= (uint64_t)base_nibble(ref.byte(s + i)) << (4 * (i & 15));
  return fits(w[0], w[1], minus ? m.r : m.f, m.len);
}
// the other site of a combined unit: of the + site q the - site, of the - site q the + site
MM_HD int64_t partner_pos(const Motif& m, int64_t q, bool minus) { return minus ? q - (m.len - 1 - m.pos) + m.pos : q - m.pos + (m.len - 1 - m.pos); }

MM_HD bool covered(uint64_t n_valid, int64_t min_coverage) { return n_valid >= (uint64_t)min_coverage; }
MM_HD bool modified(uint64_t n_mod, uint64_t n_valid, int64_t min_coverage, double min_frac) {
  return covered(n_valid, min_coverage) && (double)n_mod >= min_frac * (double)n_valid;
}

// first entry of the ascending keys[0, n) that is not below key
MM_HD int64_t lower_entry(const uint64_t* keys, int64_t n, uint64_t key) {
  int64_t a = 0, b = n;
  while (a < b) { const int64_t mid = a + (b - a) / 2; if (keys[mid] < key) a = mid + 1; else b = mid; }
  return a;
}
// the first entry of the site (contig, pos, strand), or -1 where the table has none
MM_HD int64_t site_entry(const uint64_t* keys, int64_t n, int64_t contig, int64_t pos, bool minus) {
  const uint64_t k = mmd::make_key(contig, pos, minus ? -1 : 1, 0);
  const int64_t i = lower_entry(keys, n, k);
  return i < n && mmd::key_site(keys[i]) == mmd::key_site(k) ? i : -1;
}

struct Row { uint64_t site; int32_t motif, code; uint64_t n_mod, n_canonical, n_other, n_fail; };   // site: contig << 36 | pos << 4 | (strand < 0) << 3; combined: the unit's, strand bit 0
// The rows that the segment starting at entry i of the ascending unique keys[0, n) gives: for every motif, in their order, that has an occurrence (a unit
// this segment owns, under combine) at the site, the covered rows of the applicable codes in their order, to out (null: counted only; room for MAX_MOTIFS *
// mmd::MAX_CODES); returns their number.  contig_len: the site's contig's; ref: its bytes.  Every such row is also handed to the sums of its (contig, motif,
// code) as add(motif, code, is_modified, n_valid, n_mod).
template <class R, class Add>
MM_HD int site_rows(const uint64_t* keys, const uint32_t* counts, int64_t i, int64_t n, const R& ref, int64_t contig_len, const mmd::CodeBases& cb, const Motifs& M, int64_t min_coverage,
                    double min_frac, bool combine, Row* out, Add&& add) {
  const int64_t c = mmd::key_contig(keys[i]), q = mmd::key_pos(keys[i]);
  const bool minus = mmd::key_minus(keys[i]);
  mmd::Row mine[mmd::MAX_CODES], other[mmd::MAX_CODES];
  const int n_mine = mmd::segment_rows(keys, counts, i, n, ref.byte(q), cb, 0, mine);
  int rows = 0;
  for (int32_t j = 0; j < M.n && n_mine; ++j) {
    const Motif& m = M.m[j];
    if (m.base != cb.b[mmd::key_class(mine[0].site)] || !occurs(ref, contig_len, q, minus, m)) continue;
    int n_other = 0;
    uint64_t site = keys[i] & ~(uint64_t)7;
    if (combine) {
      const int64_t p = partner_pos(m, q, minus);
      const int64_t e = site_entry(keys, n, c, p, !minus);
      if (minus && e >= 0) continue;                               // the + site has an entry: its segment owns the unit
      if (e >= 0) n_other = mmd::segment_rows(keys, counts, e, n, ref.byte(p), cb, 0, other);   // (the same codes in the same order: the complement of the partner's base is M[o] too)
      site = mmd::make_key(c, minus ? p : q, 1, 0);
    }
    for (int k = 0; k < n_mine; ++k) {
      Row r{site, j, (int32_t)mmd::key_class(mine[k].site), mine[k].n_mod, mine[k].n_canonical, mine[k].n_other, mine[k].n_fail};
      if (k < n_other) { r.n_mod += other[k].n_mod; r.n_canonical += other[k].n_canonical; r.n_other += other[k].n_other; r.n_fail += other[k].n_fail; }
      const uint64_t valid = r.n_mod + r.n_canonical + r.n_other;
      if (!covered(valid, min_coverage)) continue;
      add(j, r.code, modified(r.n_mod, valid, min_coverage, min_frac), valid, r.n_mod);
      if (out) out[rows] = r;
      ++rows;
    }
  }
  return rows;
}

}  // namespace mmt
