// The consensus of a run's primary alignments (mapDirectly --consensus; DESIGN.md section 1, "Consensus"): the sequence of the strain the reads come from, per
// contig, written once for the kernels of mm_cons.hip and for the host (plain g++: tests/test_cons_core.cpp holds it to tests/cons_ref.py).  Keys, codes, depth
// and the threshold are mm_pileup_core.hpp's (key_contig, key_pos, key_code, depth_at, site_kept), an insertion's length and bases mm_vcf_core.hpp's.
//
//   inputs     a merged --vcf table (rows (w0, w1, count), keys ascending and unique, every key valid by mmv::key_valid), the intervals (contig, first, last)
//              of every contributing alignment, the reference; D = min_depth >= 1, 0.5 <= F = min_frac <= 1, 0 <= C = min_called <= 1, a line width >= 1.
//   depth      of (c, p): the intervals on c with first <= p <= last.  p is called where depth >= D.
//   candidate  a row with depth(c, pos) >= D and site_kept(count, depth, 1, F), pos the SNV's position or the indel's shifted anchor.  Rows at one position
//              share their depth, so they are candidates together or not at all.
//   select     per contig in key order; every rule is local, none asks whether an earlier candidate was itself applied:
//                DEL  anchor a, length n, footprint [a + 1, a + n]: applied iff a + 1 > E, E the largest footprint end of all EARLIER candidate deletions of
//                     the contig, applied or not (-1: none): an exclusive prefix maximum of end keys contig << 32 | a + n, 0 for every other row (a + n >= 1).
//                     Of D1 [10, 20], D2 [15, 25] and D3 [22, 30] only D1 is applied: D2's end hides D3, which a greedy rule (bcftools consensus) would take.
//                     Abutting deletions (a2 = a1 + n1) are both applied.  Applied footprints never overlap.
//                removed(p): p lies in the footprint of an applied deletion.
//                SNV  at p: applied iff !removed(p) and no earlier candidate SNV sits at p (a 2 / 2 tie at depth 4 and F = 0.5: the lower code wins).
//                INS  at a: applied iff !removed(a) and no earlier candidate INS sits at a (AO <= DP is not guaranteed inside repeats: two can be candidates).
//                     A DEL and an INS at one anchor are both applied, and so are an SNV and an INS at one position.
//              A candidate that is not applied counts as dropped.
//   consensus  for p = 0 .. len - 1: nothing where removed(p) (whatever the depth); else one base: the applied SNV's alt, else N where p is not called, else the
//              contig's byte as the packed set holds it if that is one of A C G T, else N; then, where an INS of n is applied at p, its bases (n <= 24) or
//              n times N (a symbolic insertion: its bases are not in the key).
//   written    a contig with an interval is written iff called >= max(1, ceil(C * len)); its consensusLength is 0 otherwise.  A written contig is never
//              empty: the leftmost applied deletion's anchor is never removed.
//   text       the bytes in lines of `width`, each followed by \n, the last one (shorter or full) too: column o lands at text offset o + o / width.
//
// A position's state is one byte: REMOVED, or (the applied SNV's code + 1) << 1, or 0.  A lane policy P is mm_pileup_core.hpp's.
// Bounds: clear_footprint writes state[g0, g0 + n); emit_position writes text[text_offset(o) .. text_offset(o + ins) + 1] of a contig whose text has
// text_bytes(L) bytes, o + ins < L.
#pragma once
#include "mm_vcf_core.hpp"
#include <cmath>

namespace mmc {

// a contig's counters, in the order of PREFIX.consensus.tsv's columns behind `length`
enum Stat { ALIGNMENTS = 0, CALLED, WRITTEN, LENGTH, SNVS, DELETIONS, DELETED_BASES, INSERTIONS, INSERTED_BASES, DROPPED, STATS };
constexpr uint8_t REMOVED = 1;

MM_HD bool thresholds_ok(int64_t min_depth, double min_frac, double min_called, int64_t width) {
  return min_depth >= 1 && min_frac >= 0.5 && min_frac <= 1 && min_called >= 0 && min_called <= 1 && width >= 1;   // (a NaN fails its comparison)
}
MM_HD bool candidate(uint32_t count, int64_t depth, int64_t min_depth, double min_frac) { return depth >= min_depth && mmp::site_kept(count, depth, 1, min_frac); }
MM_HD int64_t called_needed(double min_called, int64_t len) { const int64_t k = (int64_t)std::ceil(min_called * (double)len); return k > 1 ? k : 1; }

// ---- select: row i of the candidates, prev_w0 the key word of row i - 1 (has_prev: there is one)
MM_HD bool is_snv(uint64_t w0) { return mmp::key_code(w0) < 4; }
MM_HD bool is_del(uint64_t w0) { return mmp::key_code(w0) == mmp::CODE_DEL; }
MM_HD bool is_ins(uint64_t w0) { return mmp::key_code(w0) == mmp::CODE_INS; }
MM_HD uint64_t del_end_key(uint64_t w0, uint64_t w1) { return is_del(w0) ? mmp::interval_key(mmp::key_contig(w0), mmp::key_pos(w0) + (int64_t)w1) : 0; }
MM_HD bool del_applied(uint64_t w0, uint64_t ends_before) { return mmp::interval_key(mmp::key_contig(w0), mmp::key_pos(w0) + 1) > ends_before; }
// no earlier candidate of the same class sits at the same position: codes ascend at a position, so the row before decides (an SNV's: any row there; an INS's: an INS there)
MM_HD bool first_of_class(uint64_t w0, bool has_prev, uint64_t prev_w0) {
  if (!has_prev) return true;
  return is_ins(w0) ? prev_w0 != w0 : (prev_w0 >> mmp::POS_SHIFT) != (w0 >> mmp::POS_SHIFT);
}
MM_HD bool point_applied(uint64_t w0, bool has_prev, uint64_t prev_w0, uint8_t state_at_pos) { return !(state_at_pos & REMOVED) && first_of_class(w0, has_prev, prev_w0); }
MM_HD uint8_t snv_state(uint64_t w0) { return (uint8_t)((mmp::key_code(w0) + 1) << 1); }

// the footprints of a tile's applied deletions: `mine`: this lane has one, of n positions from g0 on.  A lane clears its own short one, all lanes a long one.
template <class P> MM_HD void clear_footprint(P& p, uint8_t* state, int64_t g0, int64_t n, bool mine) {
  const bool wide = mine && n > mmp::LONG_RUN;
  if (mine && !wide) for (int64_t t = 0; t < n; ++t) state[g0 + t] = REMOVED;
  for (uint64_t left = p.ballot(wide); left; left &= left - 1) {
    uint32_t l = 0;
    while (!(left >> l & 1)) ++l;
    const int64_t lg = p.pick(g0, l), ln = p.pick(n, l);
    for (int64_t t = p.lane(); t < ln; t += P::W) state[lg + t] = REMOVED;
  }
}

// ---- positions
MM_HD int64_t out_len(uint8_t state, int64_t ins_n, bool written) { return (state & REMOVED) || !written ? 0 : 1 + ins_n; }
MM_HD uint8_t out_base(uint8_t state, int64_t depth, int64_t min_depth, uint8_t ref_byte) {
  if (state >> 1) return (uint8_t)"ACGT"[((state >> 1) - 1) & 3];
  if (depth < min_depth) return 'N';
  const uint32_t c = mmp::base_code(ref_byte);
  return c < 4 ? (uint8_t)"ACGT"[c] : (uint8_t)'N';
}
MM_HD uint8_t ins_byte(uint64_t w1, int64_t t) { return mmv::ins_len(w1) > mmv::INS_BASES_MAX ? (uint8_t)'N' : (uint8_t)"ACGT"[mmv::ins_bases(w1) >> (2 * t) & 3]; }

// ---- text
MM_HD int64_t text_offset(int64_t o, int64_t width) { return o + o / width; }
MM_HD int64_t text_bytes(int64_t len, int64_t width) { return len + (len + width - 1) / width; }
MM_HD int64_t text_lines(int64_t len, int64_t width) { return (len + width - 1) / width; }
// column o of a contig of len columns whose text starts at `text`; the column that ends a line, or the contig, writes the \n behind it
MM_HD void put(uint8_t* text, int64_t len, int64_t width, int64_t o, uint8_t b) {
  const int64_t at = text_offset(o, width);
  text[at] = b;
  if ((o + 1) % width == 0 || o + 1 == len) text[at + 1] = '\n';
}
// a tile of positions: a lane that is `live` writes its base to column o and its insertion (w1 != 0) behind it, up to LONG_RUN bases itself; all lanes write a
// longer one, which is symbolic (LONG_RUN > INS_BASES_MAX)
template <class P> MM_HD void emit_position(P& p, uint8_t* text, int64_t len, int64_t width, int64_t o, bool live, uint8_t base, uint64_t w1) {
  const int64_t n = live ? mmv::ins_len(w1) : 0;
  const bool wide = n > mmp::LONG_RUN;
  if (live) put(text, len, width, o, base);
  if (n && !wide) for (int64_t t = 0; t < n; ++t) put(text, len, width, o + 1 + t, ins_byte(w1, t));
  for (uint64_t left = p.ballot(wide); left; left &= left - 1) {
    uint32_t l = 0;
    while (!(left >> l & 1)) ++l;
    // (the contig's text: a lane of another contig of the tile writes through the picked pointer)
    uint8_t* const lt = (uint8_t*)p.pick((int64_t)text, l);
    const int64_t lo = p.pick(o, l), ln = p.pick(n, l), ll = p.pick(len, l);
    for (int64_t t = p.lane(); t < ln; t += P::W) put(lt, ll, width, lo + 1 + t, 'N');
  }
}

}  // namespace mmc
