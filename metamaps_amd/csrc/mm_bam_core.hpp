// BAM records of aligned mappings (mapDirectly --bam; DESIGN.md section 1, "BAM output"; SAM/BAM specification v1.6): the size and the bytes of one
// record, written once for the kernels of mm_bam.hip (one wavefront per record) and for the host (plain g++: tests/test_bam_core.cpp holds it to
// tests/bam_ref.py byte for byte).
//
//   record   block_size | refID pos l_read_name mapq bin n_cigar_op flag l_seq next_refID (-1) next_pos (-1) tlen (0) | read_name NUL | cigar |
//            seq (4-bit codes of =ACMGRSVTWYHKDBN, first base in the high nibble) | qual (Phred bytes, 0xFF without) | NM:i (int32) | MD:Z | CG:B,I (long CIGARs only)
//   cigar    the alignment's runs as they are (len << 4 | op; I 1, D 2, = 7, X 8).  More than 65 535 runs: the field holds l_seq S and refspan N,
//            the runs go into the CG tag (the specification's convention).
//   seq      the read as its set holds it, upper-cased; for strand - reversed, every code complemented by reversing its four bits.  A byte that is
//            not in the table is N.
//   MD       from the runs and the forward reference alone.  A counter c of matched bases: = of n adds n, I leaves it alone, every base of an X run
//            writes c, the reference base, and clears c (so consecutive mismatches are separated by 0), a D run writes c, ^, its bases, and clears c;
//            the end writes c.  A reference base is the set's byte upper-cased, a byte outside A-Z is written N.
//   walk     one pass over the runs gives the sums the checks need, the reference span and the MD text or its length.  It is defined over groups of
//            G = 64 runs whatever the number of lanes.  Run k needs c before it: with E the sum of the = lengths before k and Eb that sum at the
//            last X or D run before k, c = E - Eb; E is a prefix sum, and Eb a prefix maximum since E never falls.  The place of the run's piece of
//            text and its first reference base are prefix sums too.  A lane then writes its own run's piece.
//   checks   the rules of mm_bam_encode, numbered as BAM_RULE_*; a job that breaks one has no size.
//
// A lane policy P (the host's below, the device's in mm_bam.hip) has
//   P::W, p.lane()              as in mm_deflate.hpp; per-lane code is `for (l = p.lane(); l < n; l += P::W)`
//   p.scan_add(v, &total)       the sum of v over the lanes below this one, and over all lanes (host: 0 and v: its lanes run one by one, and the caller
//   p.scan_max(v, &total)       keeps the running value); the same for the maximum of non-negative values
// Q and R give q.byte(i), the read's byte i as stored (forward), and r.byte(j), the contig's byte j; write_record_q's Q also q.qual(i).
//
// Bounds: write_record reads ops[0, n_ops), name[0, l_name), q.byte(0 .. m - 1) and r.byte(first .. first + refspan - 1) and writes dst[0, size), size
// the value record_size gave for the same job; the checks have passed before it runs, so first >= 0 and first + refspan <= the contig's length.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef MM_HD
#if defined(__HIPCC__)
#define MM_HD __host__ __device__ inline
#else
#define MM_HD inline
#endif
#endif

namespace mmb {

constexpr uint32_t G = 64;                                        // runs per step of the walk
constexpr int64_t CIGAR_FIELD_MAX = 65535;                        // more runs than n_cigar_op holds: the CG tag
constexpr uint32_t FIXED = 36;                                    // block_size and the 32 fixed bytes behind it
constexpr uint32_t OP_I = 1, OP_D = 2, OP_N = 3, OP_S = 4, OP_EQ = 7, OP_X = 8;

enum Rule : int {                                                 // mm_bam_encode's refusals
  BAM_OK = 0,
  BAM_RULE_SET = 1,                                               // a read or contig outside its set
  BAM_RULE_STRAND = 2,                                            // a strand that is not +1 / -1, or flag & 0x10 that disagrees with it
  BAM_RULE_NAME = 3,                                              // a name of 0 or more than 254 bytes
  BAM_RULE_RUN = 4,                                               // a run whose op is not 1, 2, 7 or 8, or whose length is 0
  BAM_RULE_READ = 5,                                              // the = X I runs do not add up to the read's length
  BAM_RULE_SPAN = 6,                                              // first < 0, or first and the = X D runs pass the contig's end
  BAM_RULE_DIST = 7,                                              // the X I D runs do not add up to dist
};
MM_HD const char* rule_text(int rule) {
  switch (rule) {
    case BAM_RULE_SET: return "rule 1: the read or the contig lies outside its set";
    case BAM_RULE_STRAND: return "rule 2: the strand is not +1 or -1, or flag & 0x10 disagrees with it";
    case BAM_RULE_NAME: return "rule 3: the name has 0 or more than 254 bytes";
    case BAM_RULE_RUN: return "rule 4: a run's op is not 1, 2, 7 or 8, or its length is 0";
    case BAM_RULE_READ: return "rule 5: the = X I runs do not add up to the read's length";
    case BAM_RULE_SPAN: return "rule 6: first is negative, or first plus the = X D runs passes the contig's end";
    case BAM_RULE_DIST: return "rule 7: the X I D runs do not add up to dist";
    default: return "no rule";
  }
}

struct Job {
  const uint32_t* ops; int64_t n_ops;                             // the runs
  const char* name; int32_t l_name;                               // without the NUL
  int64_t first; int32_t m, refid, strand, dist;
  uint16_t flag; uint8_t mapq;
};
struct Walk { int64_t q, r, edits, md_len; uint32_t bad_run; };   // sums of = X I, of = X D, of X I D; the MD text's bytes; a run of rule 4

MM_HD uint32_t reg2bin(int64_t beg, int64_t end) {                // the specification's section 5.3
  --end;
  if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
  return 0;
}
MM_HD uint32_t dec_width(uint64_t v) { uint32_t w = 1; while (v >= 10) { v /= 10; ++w; } return w; }
MM_HD uint32_t put_dec(uint8_t* o, uint64_t v) {                  // v in decimal at o; its width
  const uint32_t w = dec_width(v);
  for (uint32_t k = w; k-- > 0;) { o[k] = (uint8_t)('0' + v % 10); v /= 10; }
  return w;
}
MM_HD uint8_t upper(uint8_t b) { return b >= 'a' && b <= 'z' ? (uint8_t)(b - 32) : b; }
MM_HD uint8_t md_base(uint8_t b) { b = upper(b); return b >= 'A' && b <= 'Z' ? b : (uint8_t)'N'; }
MM_HD uint32_t nt16_code(uint8_t b) {                             // the place of the upper-cased byte in =ACMGRSVTWYHKDBN, N (15) for any other
  switch (upper(b)) {
    case '=': return 0; case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5; case 'S': return 6; case 'V': return 7;
    case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11; case 'K': return 12; case 'D': return 13; case 'B': return 14;
    default: return 15;
  }
}
MM_HD uint32_t nt16_complement(uint32_t c) { return ((c & 1) << 3) | ((c & 2) << 1) | ((c & 4) >> 1) | ((c & 8) >> 3); }
template <class Q> MM_HD uint32_t oriented_code(const Q& q, int32_t m, int32_t strand, int32_t i) {   // base i of the record's SEQ
  return strand < 0 ? nt16_complement(nt16_code(q.byte(m - 1 - i))) : nt16_code(q.byte(i));
}

// A read source Q with qualities also gives q.qual(i), the stored quality of the read's base i (forward): Phred 0..93, 0xFF for "no quality".
constexpr uint8_t QUAL_NONE = 0xFF;
template <class Q> MM_HD uint8_t oriented_qual(const Q& q, int64_t m, int32_t strand, int64_t i) {   // of base i of the oriented read
  return q.qual(strand < 0 ? m - 1 - i : i);
}
template <class Q> struct NoQual {                                // a source of bytes alone: every base is without quality
  const Q& q;
  MM_HD uint8_t byte(int64_t i) const { return q.byte(i); }
  MM_HD uint8_t qual(int64_t) const { return QUAL_NONE; }
};
struct QualBytes {                                                // the host's source: the read's bytes and its stored qualities (null: none)
  const uint8_t* b; const uint8_t* q;
  uint8_t byte(int64_t i) const { return b[i]; }
  uint8_t qual(int64_t i) const { return q ? q[i] : QUAL_NONE; }
};

// rule 1, asked of every job before anything is read through its indexes; the other rules are asked of the jobs that have a record (dist >= 0 and a
// read that is not empty)
MM_HD int check_set(int64_t read, int64_t n_reads, int64_t contig, int64_t n_contigs) {
  return read < 0 || read >= n_reads || contig < 0 || contig >= n_contigs ? BAM_RULE_SET : BAM_OK;
}
MM_HD int check_head(int32_t strand, uint32_t flag, int64_t l_name) {   // rules 2 and 3
  if ((strand != 1 && strand != -1) || ((flag & 0x10u) != 0) != (strand < 0)) return BAM_RULE_STRAND;
  if (l_name < 1 || l_name > 254) return BAM_RULE_NAME;
  return BAM_OK;
}
// rules 4 to 7, from the walk's sums
MM_HD int check_walk(const Walk& w, int64_t m, int64_t first, int64_t contig_len, int64_t dist) {
  if (w.bad_run) return BAM_RULE_RUN;
  if (w.q != m) return BAM_RULE_READ;
  if (first < 0 || first + w.r > contig_len) return BAM_RULE_SPAN;
  if (w.edits != dist) return BAM_RULE_DIST;
  return BAM_OK;
}

// the runs once: the sums, and the MD text's length; WRITE: the text itself to md (md_len bytes, no NUL).  Every lane returns the same Walk.
template <bool WRITE, class P, class R> MM_HD Walk md_walk(P& p, const R& ref, const uint32_t* ops, int64_t n_ops, int64_t first, uint8_t* md) {
  int64_t E = 0, Eb = 0, rsum = 0, qsum = 0, edits = 0, at = 0, bad = 0;   // the running values: the same in every lane
  for (int64_t base = 0; base < n_ops; base += G)
    for (uint32_t l = p.lane(); l < G; l += P::W) {
      const int64_t k = base + l;
      const bool in = k < n_ops;
      const uint32_t w = in ? ops[k] : 0, op = w & 15u;
      const int64_t len = (int64_t)(w >> 4);
      const bool good = in && len > 0 && (op == OP_I || op == OP_D || op == OP_EQ || op == OP_X);
      const bool brk = good && (op == OP_X || op == OP_D);
      int64_t tot;
      const int64_t e = E + p.scan_add(good && op == OP_EQ ? len : 0, &tot); E += tot;
      int64_t eb = p.scan_max(brk ? e : 0, &tot); eb = eb > Eb ? eb : Eb; Eb = tot > Eb ? tot : Eb;
      const int64_t rj = rsum + p.scan_add(good && op != OP_I ? len : 0, &tot); rsum += tot;
      (void)p.scan_add(good && op != OP_D ? len : 0, &tot); qsum += tot;
      (void)p.scan_add(good && op != OP_EQ ? len : 0, &tot); edits += tot;
      (void)p.scan_add(in && !good ? 1 : 0, &tot); bad += tot;
      const uint64_t c = (uint64_t)(e - eb);
      const int64_t piece = !brk ? 0 : op == OP_X ? dec_width(c) + 1 + 2 * (len - 1) : dec_width(c) + 1 + len;
      const int64_t mine = at + p.scan_add(piece, &tot); at += tot;
      if (WRITE && brk) {
        uint8_t* o = md + mine;
        o += put_dec(o, c);
        if (op == OP_D) *o++ = '^';
        for (int64_t i = 0; i < len; ++i) { if (op == OP_X && i) *o++ = '0'; *o++ = md_base(ref.byte(first + rj + i)); }
      }
    }
  const uint64_t c = (uint64_t)(E - Eb);
  if (WRITE && p.lane() == 0) put_dec(md + at, c);
  Walk out;
  out.q = qsum; out.r = rsum; out.edits = edits; out.md_len = at + dec_width(c); out.bad_run = bad != 0;
  return out;
}

MM_HD bool long_cigar(int64_t n_ops) { return n_ops > CIGAR_FIELD_MAX; }
MM_HD int64_t record_size(int64_t l_name, int64_t m, int64_t n_ops, int64_t md_len) {
  const int64_t field = long_cigar(n_ops) ? 2 : n_ops;
  return FIXED + l_name + 1 + 4 * field + (m + 1) / 2 + m + 7 + 3 + md_len + 1 + (long_cigar(n_ops) ? 8 + 4 * n_ops : 0);
}
MM_HD void put32(uint8_t* o, uint32_t v) { o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16); o[3] = (uint8_t)(v >> 24); }

// the record of a job whose checks have passed, at dst (any byte offset: everything is stored by bytes); returns its size
// (QUAL is the oriented read's qualities, 0xFF on every base of a read without)
template <class P, class Q, class R> MM_HD int64_t write_record_q(P& p, const Job& j, const Q& q, const R& ref, uint8_t* dst) {
  const bool lc = long_cigar(j.n_ops);
  const int64_t n_field = lc ? 2 : j.n_ops, m = j.m;
  uint8_t* const name = dst + FIXED;
  uint8_t* const cigar = name + j.l_name + 1;
  uint8_t* const seq = cigar + 4 * n_field;
  uint8_t* const qual = seq + (m + 1) / 2;
  uint8_t* const nm = qual + m;
  uint8_t* const md = nm + 7;
  const Walk w = md_walk<true>(p, ref, j.ops, j.n_ops, j.first, md + 3);
  const int64_t size = record_size(j.l_name, m, j.n_ops, w.md_len);
  for (uint32_t l = p.lane(); l < 9; l += P::W) {
    const uint32_t v = l == 0 ? (uint32_t)(size - 4) : l == 1 ? (uint32_t)j.refid : l == 2 ? (uint32_t)j.first
                     : l == 3 ? (uint32_t)(j.l_name + 1) | (uint32_t)j.mapq << 8 | reg2bin(j.first, j.first + w.r) << 16
                     : l == 4 ? (uint32_t)n_field | (uint32_t)j.flag << 16 : l == 5 ? (uint32_t)m : l == 8 ? 0u : 0xFFFFFFFFu;
    put32(dst + 4 * l, v);
  }
  for (int64_t i = p.lane(); i <= j.l_name; i += P::W) name[i] = i < j.l_name ? (uint8_t)j.name[i] : 0;
  if (lc) for (uint32_t l = p.lane(); l < 2; l += P::W) put32(cigar + 4 * l, l == 0 ? (uint32_t)m << 4 | OP_S : (uint32_t)w.r << 4 | OP_N);
  else for (int64_t i = p.lane(); i < 4 * j.n_ops; i += P::W) cigar[i] = (uint8_t)(j.ops[i >> 2] >> (8 * (i & 3)));
  for (int64_t i = p.lane(); i < (m + 1) / 2; i += P::W)
    seq[i] = (uint8_t)(oriented_code(q, j.m, j.strand, (int32_t)(2 * i)) << 4 | (2 * i + 1 < m ? oriented_code(q, j.m, j.strand, (int32_t)(2 * i + 1)) : 0u));
  for (int64_t i = p.lane(); i < m; i += P::W) qual[i] = oriented_qual(q, m, j.strand, i);
  for (uint32_t l = p.lane(); l < 7; l += P::W) nm[l] = l == 0 ? 'N' : l == 1 ? 'M' : l == 2 ? 'i' : (uint8_t)((uint32_t)j.dist >> (8 * (l - 3)));
  for (uint32_t l = p.lane(); l < 4; l += P::W) { if (l < 3) md[l] = l == 0 ? 'M' : l == 1 ? 'D' : 'Z'; else md[3 + w.md_len] = 0; }
  if (lc) {
    uint8_t* const cg = md + 3 + w.md_len + 1;
    for (uint32_t l = p.lane(); l < 8; l += P::W) cg[l] = l == 0 ? 'C' : l == 1 ? 'G' : l == 2 ? 'B' : l == 3 ? 'I' : (uint8_t)((uint32_t)j.n_ops >> (8 * (l - 4)));
    for (int64_t i = p.lane(); i < 4 * j.n_ops; i += P::W) cg[8 + i] = (uint8_t)(j.ops[i >> 2] >> (8 * (i & 3)));
  }
  return size;
}

// the same of a read source without qualities
template <class P, class Q, class R> MM_HD int64_t write_record(P& p, const Job& j, const Q& q, const R& ref, uint8_t* dst) {
  return write_record_q(p, j, NoQual<Q>{q}, ref, dst);
}

// the host's lane policy: one lane
struct HostLanes {
  static constexpr uint32_t W = 1;
  uint32_t lane() const { return 0; }
  int64_t scan_add(int64_t v, int64_t* total) const { *total = v; return 0; }
  int64_t scan_max(int64_t v, int64_t* total) const { *total = v; return 0; }
};

}  // namespace mmb
