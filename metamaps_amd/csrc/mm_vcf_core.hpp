// The alleles of a run's primary alignments (mapDirectly --vcf; DESIGN.md section 1, "VCF"): what every alignment says about the reference as SNV, deletion and
// insertion alleles that are canonical across reads, written once for the kernels of mm_vcf.hip (one wavefront per job) and for the host (plain g++:
// tests/test_vcf_core.cpp holds it to tests/vcf_ref.py).  Runs, the oriented read Q, codes, the lane policy, depth and the checks are mm_pileup_core.hpp's.
//
//   walk     r = first, i = 0, last = first + (the = X D runs) - 1:
//              = of n   nothing                                                                              r += n, i += n
//              X of n   an SNV (contig, r + t, code(Q[i + t])) per base whose code is A C G T                 r += n, i += n
//              D of n   a DEL of n anchored at a = r - 1, where first < r and r + n <= last                   r += n
//              I of n   an INS of n with the bases S = Q[i .. i + n), all of them A C G T, anchored at
//                       a = r - 1, where first < r <= last                                                    i += n
//            An indel run without an aligned reference position on both sides (the first and the last run of a job, and a run that only other
//            indel runs separate from an end) is an alignment edge, not an allele.
//   shift    every indel is left-aligned before it is keyed (the step of `bcftools norm`), at most NORM_MAX times:
//              DEL   while a > first and ref[a] == ref[a + n], both A C G T (upper-cased): a -= 1
//              INS   while a > first and ref[a] == the last base of S, ref[a] one of A C G T: S turns right by one and a -= 1; after s steps
//                    S'[j] = S[(j - s) mod n]: index arithmetic on the read
//            a > first keeps every allele inside [first, last]; a read whose alignment starts inside a repeat may leave its indel further right.
//   floor    mm_vcf_events_q's min_base_quality Qm > 0, by mm_pileup_core.hpp's rules: an SNV is kept iff q(i + t) >= Qm, a DEL iff the read's bases on
//            either side of the gap have q >= Qm, an INS iff every base of S has.  It is asked before the shift, which acts on the alleles that were
//            kept; an allele that is not kept is skipped.  An insertion's minimum is taken by its own lane, as its bases are read for the key.
//   key      two words, ordered by (w0, w1).  w0 = mmp::make_key(contig, pos, code): code the alt's 0-3 for an SNV, CODE_DEL, CODE_INS; pos the SNV's
//            position or the shifted anchor.  w1: 0 (SNV); n (DEL); n << 48 | the bases, 2 bits each, base j at bits 2j (INS, n <= 24); n << 48 (INS,
//            n > 24: a symbolic insertion, equal lengths at equal anchors count together).
//   skipped  an X base outside A C G T, an insertion holding one, an edge run that is neither the first nor the last, an allele under the floor: (SKIP,
//            SKIP), which sorts last.
//   checks   mm_bam_encode's rules 1, 2, 4, 5, 6 as mmp::count_job applies them, then rule 8: an I or D run that is neither first nor last has 2^16
//            bases or more.
//   finish   depth = mmp::depth_at(contig, pos); kept where mmp::site_kept; a kept allele carries ref[pos .. pos + WINDOW), clipped at the contig's end
//            (zero bytes beyond): REF of every line can be printed from it.
//
// A lane policy P is mm_pileup_core.hpp's.  Q gives q.byte(i), the read's byte i as its set holds it (forward), and for emit_job_q q.qual(i); R gives r.byte(pos), the contig's byte.
// Bounds: count_job reads ops[0, n_ops); emit_job reads the same, q.byte(0 .. m - 1) and r.byte(first .. last), and writes w0 and w1 [0, alleles),
// alleles the value count_job gave for the same job, whose checks have passed.
#pragma once
#include "mm_pileup_core.hpp"

namespace mmv {

constexpr int64_t NORM_MAX = 256;                                 // left shifts of one indel at most: a constant of the definition
constexpr int64_t INS_BASES_MAX = 24;                             // an insertion's bases are part of its key up to here; a DEL prints its bases up to here
constexpr int64_t INDEL_MAX = (int64_t)1 << 16;                   // an indel is shorter
constexpr int LEN_SHIFT = 48, WINDOW = 25;
constexpr uint64_t SKIP = ~0ull;
constexpr int VCF_RULE_INDEL = 8;

MM_HD const char* rule_text(int rule) { return rule == VCF_RULE_INDEL ? "rule 8: an I or D run between other runs has 2^16 bases or more" : mmp::rule_text(rule); }

struct Allele { uint64_t w0, w1; };
MM_HD int64_t ins_len(uint64_t w1) { return (int64_t)(w1 >> LEN_SHIFT); }
MM_HD uint64_t ins_bases(uint64_t w1) { return w1 & (((uint64_t)1 << LEN_SHIFT) - 1); }

MM_HD bool indel_op(uint32_t op) { return op == mmb::OP_I || op == mmb::OP_D; }
// what run k of n_ops adds to the job's bound of alleles: its bases (X), 1 (an I or D run that is neither first nor last)
MM_HD int64_t run_alleles(const mmp::Run& x, int64_t k, int64_t n_ops) {
  return !x.good ? 0 : x.op == mmb::OP_X ? x.len : indel_op(x.op) && k > 0 && k + 1 < n_ops ? 1 : 0;
}

// the rules of a job that is used; *alleles: what emit_job will write; *indels: how many of them come from I or D runs
template <class P> MM_HD int count_job(P& p, int64_t read, int64_t n_reads, int64_t contig, int64_t n_contigs, int32_t strand, const int32_t* q_len, const int32_t* r_len,
                                       int64_t first, const uint32_t* ops, int64_t n_ops, int64_t* alleles, int64_t* indels) {
  *alleles = 0; *indels = 0;
  int64_t events;
  const int rule = mmp::count_job(p, read, n_reads, contig, n_contigs, strand, q_len, r_len, first, ops, n_ops, &events);
  if (rule) return rule;
  int64_t al = 0, ind = 0, big = 0;
  for (int64_t base = 0; base < n_ops; base += P::W) {
    const int64_t k = base + p.lane();
    const mmp::Run x = mmp::run_of(ops, k, n_ops);
    const int64_t mine = run_alleles(x, k, n_ops);
    const bool indel = mine && indel_op(x.op);
    int64_t tot;
    (void)p.scan_add(mine, &tot); al += tot;
    (void)p.scan_add(indel ? 1 : 0, &tot); ind += tot;
    (void)p.scan_add(indel && x.len >= INDEL_MAX ? 1 : 0, &tot); big += tot;
  }
  if (big) return VCF_RULE_INDEL;
  *alleles = al; *indels = ind;
  return mmb::BAM_OK;
}

// the allele of an I or D run of n at contig position r and read index i of a job on [first, last]
// (qmin: the quality floor, asked before the shift; an allele that is not kept is skipped)
template <class Q, class R> MM_HD Allele indel_allele(const Q& q, int64_t m, int32_t strand, const R& ref, int64_t contig, int64_t first, int64_t last, uint32_t op, int64_t n,
                                                      int64_t r, int64_t i, int32_t qmin) {
  const Allele skip{SKIP, SKIP};
  int64_t a = r - 1;
  if (op == mmb::OP_D) {
    if (!(first < r && r + n <= last)) return skip;
    if (qmin > 0 && !mmp::del_kept(q, m, strand, i, qmin)) return skip;
    for (int64_t s = 0; s < NORM_MAX && a > first; ++s) {
      const uint32_t c = mmp::base_code(ref.byte(a));
      if (c >= 4 || c != mmp::base_code(ref.byte(a + n))) break;
      --a;
    }
    return Allele{mmp::make_key(contig, a, mmp::CODE_DEL), (uint64_t)n};
  }
  if (!(first < r && r <= last)) return skip;
  for (int64_t t = 0; t < n; ++t) if (mmp::oriented_code(q, m, strand, i + t) >= 4) return skip;
  if (qmin > 0) for (int64_t t = 0; t < n; ++t) if (mmb::oriented_qual(q, m, strand, i + t) < qmin) return skip;
  int64_t s = 0, tail = n - 1;                                    // tail: the index in S of the last base of S' = (n - 1 - s) mod n
  for (; s < NORM_MAX && a > first; ++s) {
    const uint32_t c = mmp::base_code(ref.byte(a));
    if (c >= 4 || c != mmp::oriented_code(q, m, strand, i + tail)) break;
    --a; tail = tail ? tail - 1 : n - 1;
  }
  uint64_t w1 = (uint64_t)n << LEN_SHIFT;
  if (n <= INS_BASES_MAX) {
    int64_t from = tail + 1 == n ? 0 : tail + 1;                  // S'[0] = S[(0 - s) mod n] = the base behind the tail
    for (int64_t j = 0; j < n; ++j) { w1 |= (uint64_t)mmp::oriented_code(q, m, strand, i + from) << (2 * j); from = from + 1 == n ? 0 : from + 1; }
  }
  return Allele{mmp::make_key(contig, a, mmp::CODE_INS), w1};
}
template <class Q> MM_HD Allele snv_allele(const Q& q, int64_t m, int32_t strand, int64_t contig, int64_t pos, int64_t i, int32_t qmin) {
  const uint32_t c = mmp::oriented_code(q, m, strand, i);
  return c < 4 && (qmin <= 0 || mmb::oriented_qual(q, m, strand, i) >= qmin) ? Allele{mmp::make_key(contig, pos, c), 0} : Allele{SKIP, SKIP};
}

// the alleles of a job whose checks have passed to w0 and w1 [0, alleles), in the order of the walk; returns their number (the same in every lane)
template <class P, class Q, class R> MM_HD int64_t emit_job_q(P& p, const Q& q, int64_t m, int32_t strand, const R& ref, int64_t contig, int64_t first, const uint32_t* ops,
                                                              int64_t n_ops, int32_t qmin, uint64_t* w0, uint64_t* w1) {
  const int64_t last = first + mmp::count_walk(p, ops, n_ops).r - 1;
  int64_t rsum = 0, isum = 0, at = 0;                             // the running values: the same in every lane
  for (int64_t base = 0; base < n_ops; base += P::W) {
    const int64_t k = base + p.lane();
    const mmp::Run x = mmp::run_of(ops, k, n_ops);
    const int64_t al = run_alleles(x, k, n_ops);
    int64_t tot;
    const int64_t r = first + rsum + p.scan_add(x.good && x.op != mmb::OP_I ? x.len : 0, &tot); rsum += tot;
    const int64_t i = isum + p.scan_add(x.good && x.op != mmb::OP_D ? x.len : 0, &tot); isum += tot;
    const int64_t o = at + p.scan_add(al, &tot); at += tot;
    const bool wide = al > mmp::LONG_RUN;                         // (an X run: an indel run gives one allele)
    if (al && !wide) {                                            // a short run: its own lane writes it, and shifts its indel
      if (x.op == mmb::OP_X) for (int64_t t = 0; t < al; ++t) { const Allele e = snv_allele(q, m, strand, contig, r + t, i + t, qmin); w0[o + t] = e.w0; w1[o + t] = e.w1; }
      else { const Allele e = indel_allele(q, m, strand, ref, contig, first, last, x.op, x.len, r, i, qmin); w0[o] = e.w0; w1[o] = e.w1; }
    }
    for (uint64_t left = p.ballot(wide); left; left &= left - 1) {   // the long X runs of the tile, one after the other, by all lanes
      uint32_t l = 0;
      while (!(left >> l & 1)) ++l;
      const int64_t lr = p.pick(r, l), li = p.pick(i, l), lo = p.pick(o, l), ln = p.pick(al, l);
      for (int64_t t = p.lane(); t < ln; t += P::W) { const Allele e = snv_allele(q, m, strand, contig, lr + t, li + t, qmin); w0[lo + t] = e.w0; w1[lo + t] = e.w1; }
    }
  }
  return at;
}

// the same without a floor, of a read source without qualities
template <class P, class Q, class R> MM_HD int64_t emit_job(P& p, const Q& q, int64_t m, int32_t strand, const R& ref, int64_t contig, int64_t first, const uint32_t* ops,
                                                            int64_t n_ops, uint64_t* w0, uint64_t* w1) {
  return emit_job_q(p, mmb::NoQual<Q>{q}, m, strand, ref, contig, first, ops, n_ops, 0, w0, w1);
}

// what mm_vcf_merge's output and mm_vcf_finish's input hold: a key of the definition on a contig of contig_len bases
MM_HD bool key_valid(uint64_t w0, uint64_t w1, int64_t contig_len) {
  const int64_t pos = mmp::key_pos(w0);
  const uint32_t code = mmp::key_code(w0);
  if (pos >= contig_len) return false;
  if (code < 4) return w1 == 0;
  if (code == mmp::CODE_DEL) return w1 >= 1 && w1 < (uint64_t)INDEL_MAX && pos + (int64_t)w1 < contig_len;
  if (code != mmp::CODE_INS) return false;
  const int64_t n = ins_len(w1);
  if (n < 1) return false;
  return n > INS_BASES_MAX ? ins_bases(w1) == 0 : (ins_bases(w1) >> (2 * n)) == 0;
}
MM_HD int64_t window_len(int64_t pos, int64_t contig_len) { return contig_len - pos < WINDOW ? contig_len - pos : WINDOW; }

}  // namespace mmv
