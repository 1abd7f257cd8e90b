// The pileup of a run's primary alignments (mapDirectly --pileup; DESIGN.md section 1, "Pileup"): what every alignment says about the columns of the
// reference, written once for the kernels of mm_pileup.hip (one wavefront per job) and for the host (plain g++: tests/test_pileup_core.cpp holds it to
// tests/pileup_ref.py).
//
//   runs     an aligned job has first (the contig position of its first base) and the runs mm_alignment_fetch gives: len << 4 | op with I = 1, D = 2,
//            = = 7, X = 8; for strand -1 they are those of the reverse-complemented read along the forward contig.
//   walk     r = first, i = 0 (the index in the oriented read Q):
//              = of n   no event                                                          r += n, i += n
//              X of n   (contig, r + t, code(Q[i + t])) for t < n                          r += n, i += n
//              D of n   (contig, r + t, DEL) for t < n                                     r += n
//              I of n   ONE event (contig, r > first ? r - 1 : first, INS)                 i += n
//            An insertion sits on the base before it (VCF's anchor), a leading one on `first`: every event lies in [first, last].
//   code     of the upper-cased read byte: A 0, C 1, G 2, T 3, anything else N = 4; DEL = 5, INS = 6.  The complement of N is N; a strand -1 job
//            reads its bases from the read's end and complements them.
//   key      contig << 35 | pos << 3 | code: keys order by contig, position, code.  2^29 contigs at most.
//   depth    of (contig, pos): the alignments on that contig with first <= pos <= last.  With the starts contig << 32 | first and the ends
//            contig << 32 | last both ascending it is (starts <= x) - (ends < x) for x = contig << 32 | pos: two binary searches (depth_at).
//   floor    mm_pileup_events_q's min_base_quality Qm > 0, with q(i) the quality of base i of the oriented read (mmb::oriented_qual; "no quality" is 255
//            and passes every floor): the event of an X run at read index i + t is kept iff q(i + t) >= Qm; the n events of a D run met at read index
//            i together iff min(q(i - 1) if i > 0, q(i) if i < m) >= Qm; the event of an I run iff min q(i .. i + n - 1) >= Qm.  An event that is not
//            kept keeps its place and holds DROPPED, which sorts behind every key and is cut off the table.  Intervals and depth are untouched.
//   checks   mm_bam_encode's rules 1, 2 (the strand), 4, 5 and 6 under its numbers (mm_bam_core.hpp): after them every read index of the walk
//            is inside the read and every position inside the contig.
//
// The walk is defined over tiles of P::W runs, one run per lane.  A lane policy P (the host's below, the device's in mm_pileup.hip) has
//   P::W, p.lane()            the lanes of a tile and this lane's number (host: 1 and 0)
//   p.scan_add(v, &total)     the sum of v over the lanes below this one, and over all lanes (host: 0 and v)
//   p.ballot(b)               bit l: lane l's b (host: bit 0)
//   p.pick(v, l)              lane l's v (host: v)
// Q gives q.byte(i), the read's byte i as its set holds it (forward); emit_job_q's Q also q.qual(i), its stored quality (mm_bam_core.hpp).
//
// Bounds: count_job reads ops[0, n_ops); emit_job reads the same and q.byte(0 .. m - 1) and writes out[0, events), events the value count_job gave
// for the same job, whose checks have passed.
#pragma once
#include "mm_bam_core.hpp"

namespace mmp {

constexpr uint32_t CODE_N = 4, CODE_DEL = 5, CODE_INS = 6, N_CODES = 7;
constexpr int POS_SHIFT = 3, CONTIG_SHIFT = 35;
constexpr int64_t MAX_CONTIGS = (int64_t)1 << 29;
constexpr uint64_t DROPPED = ~0ull;                               // in the place of an event under the quality floor: code 7, which no key has; sorts last
constexpr int64_t LONG_RUN = 64;                                  // a run with more events is expanded by all lanes of the tile

MM_HD uint64_t make_key(int64_t contig, int64_t pos, uint32_t code) { return (uint64_t)contig << CONTIG_SHIFT | (uint64_t)pos << POS_SHIFT | code; }
MM_HD int64_t key_contig(uint64_t key) { return (int64_t)(key >> CONTIG_SHIFT); }
MM_HD int64_t key_pos(uint64_t key) { return (int64_t)(key >> POS_SHIFT & 0xFFFFFFFFull); }
MM_HD uint32_t key_code(uint64_t key) { return (uint32_t)(key & 7u); }
MM_HD char code_letter(uint32_t code) { return "ACGTN-+?"[code & 7u]; }   // the `alt` column of PREFIX.pileup

MM_HD uint32_t base_code(uint8_t b) {
  switch (mmb::upper(b)) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; default: return CODE_N; }
}
MM_HD uint32_t complement(uint32_t c) { return c < 4 ? 3 - c : CODE_N; }
template <class Q> MM_HD uint32_t oriented_code(const Q& q, int64_t m, int32_t strand, int64_t i) {   // base i of the oriented read
  return strand < 0 ? complement(base_code(q.byte(m - 1 - i))) : base_code(q.byte(i));
}

MM_HD const char* rule_text(int rule) {
  return rule == mmb::BAM_RULE_STRAND ? "rule 2: the strand is not +1 or -1" : mmb::rule_text(rule);
}

struct Run { uint32_t op; int64_t len; bool good; };
MM_HD Run run_of(const uint32_t* ops, int64_t k, int64_t n_ops) {
  Run x;
  const uint32_t w = k < n_ops ? ops[k] : 0;
  x.op = w & 15u; x.len = (int64_t)(w >> 4);
  x.good = k < n_ops && x.len > 0 && (x.op == mmb::OP_I || x.op == mmb::OP_D || x.op == mmb::OP_EQ || x.op == mmb::OP_X);
  return x;
}
MM_HD int64_t run_events(const Run& x) { return !x.good ? 0 : x.op == mmb::OP_X || x.op == mmb::OP_D ? x.len : x.op == mmb::OP_I ? 1 : 0; }

struct Count { int64_t q, r, events; bool bad_run; };             // sums of = X I and of = X D; the job's events; a run of rule 4
// the runs once: every lane returns the same sums
template <class P> MM_HD Count count_walk(P& p, const uint32_t* ops, int64_t n_ops) {
  int64_t q = 0, r = 0, ev = 0, bad = 0;
  for (int64_t base = 0; base < n_ops; base += P::W) {
    const int64_t k = base + p.lane();
    const Run x = run_of(ops, k, n_ops);
    int64_t tot;
    (void)p.scan_add(x.good && x.op != mmb::OP_D ? x.len : 0, &tot); q += tot;
    (void)p.scan_add(x.good && x.op != mmb::OP_I ? x.len : 0, &tot); r += tot;
    (void)p.scan_add(run_events(x), &tot); ev += tot;
    (void)p.scan_add(k < n_ops && !x.good ? 1 : 0, &tot); bad += tot;
  }
  Count c;
  c.q = q; c.r = r; c.events = ev; c.bad_run = bad != 0;
  return c;
}
// the rules of a job that is used, in the order of their numbers; *events: what emit_job will write
template <class P> MM_HD int count_job(P& p, int64_t read, int64_t n_reads, int64_t contig, int64_t n_contigs, int32_t strand, const int32_t* q_len, const int32_t* r_len,
                                       int64_t first, const uint32_t* ops, int64_t n_ops, int64_t* events) {
  *events = 0;
  if (mmb::check_set(read, n_reads, contig, n_contigs)) return mmb::BAM_RULE_SET;
  if (strand != 1 && strand != -1) return mmb::BAM_RULE_STRAND;
  const Count c = count_walk(p, ops, n_ops);
  if (c.bad_run) return mmb::BAM_RULE_RUN;
  if (c.q != q_len[read]) return mmb::BAM_RULE_READ;
  if (first < 0 || first + c.r > r_len[contig]) return mmb::BAM_RULE_SPAN;
  *events = c.events;
  return mmb::BAM_OK;
}

// the D run met at read index i of the oriented read: the read's bases on either side of the gap
template <class Q> MM_HD bool del_kept(const Q& q, int64_t m, int32_t strand, int64_t i, int32_t qmin) {
  return (i <= 0 || mmb::oriented_qual(q, m, strand, i - 1) >= qmin) && (i >= m || mmb::oriented_qual(q, m, strand, i) >= qmin);
}

// the events of a job whose checks have passed to out[0, events), in the order of the walk; returns their number (the same in every lane).  Under
// a floor qmin > 0 an event that is not kept leaves DROPPED in its place: count_job's number is that of the places.
template <class P, class Q> MM_HD int64_t emit_job_q(P& p, const Q& q, int64_t m, int32_t strand, int64_t contig, int64_t first, const uint32_t* ops, int64_t n_ops, int32_t qmin,
                                                     uint64_t* out) {
  int64_t rsum = 0, isum = 0, at = 0;                             // the running values: the same in every lane
  for (int64_t base = 0; base < n_ops; base += P::W) {
    const Run x = run_of(ops, base + p.lane(), n_ops);
    const int64_t ev = run_events(x);
    int64_t tot;
    const int64_t r = first + rsum + p.scan_add(x.good && x.op != mmb::OP_I ? x.len : 0, &tot); rsum += tot;
    const int64_t i = isum + p.scan_add(x.good && x.op != mmb::OP_D ? x.len : 0, &tot); isum += tot;
    const int64_t o = at + p.scan_add(ev, &tot); at += tot;
    const bool ins = x.good && x.op == mmb::OP_I;
    const bool wide = ev > LONG_RUN || (qmin > 0 && ins && x.len > LONG_RUN);   // (under a floor a long insertion's minimum is taken by all lanes)
    if (ev && !wide) {                                            // a short run: its own lane writes it
      if (ins) {
        bool keep = true;
        if (qmin > 0) for (int64_t t = 0; t < x.len; ++t) keep = keep && mmb::oriented_qual(q, m, strand, i + t) >= qmin;
        out[o] = keep ? make_key(contig, r > first ? r - 1 : first, CODE_INS) : DROPPED;
      } else if (x.op == mmb::OP_D) {
        const bool keep = qmin <= 0 || del_kept(q, m, strand, i, qmin);
        for (int64_t t = 0; t < ev; ++t) out[o + t] = keep ? make_key(contig, r + t, CODE_DEL) : DROPPED;
      } else
        for (int64_t t = 0; t < ev; ++t) out[o + t] = qmin <= 0 || mmb::oriented_qual(q, m, strand, i + t) >= qmin ? make_key(contig, r + t, oriented_code(q, m, strand, i + t)) : DROPPED;
    }
    for (uint64_t left = p.ballot(wide); left; left &= left - 1) {   // the long runs of the tile, one after the other, by all lanes
      uint32_t l = 0;
      while (!(left >> l & 1)) ++l;
      const int64_t lr = p.pick(r, l), li = p.pick(i, l), lo = p.pick(o, l), ln = p.pick(ev, l), lop = p.pick((int64_t)x.op, l);
      if (lop == (int64_t)mmb::OP_I) {                              // (qmin > 0) one event, kept iff no lane met a base below the floor
        const int64_t n = p.pick(x.len, l);
        bool low = false;
        for (int64_t t = p.lane(); t < n; t += P::W) low = low || mmb::oriented_qual(q, m, strand, li + t) < qmin;
        const bool drop = p.ballot(low) != 0;
        if (p.lane() == 0) out[lo] = drop ? DROPPED : make_key(contig, lr > first ? lr - 1 : first, CODE_INS);
        continue;
      }
      const bool del = lop == (int64_t)mmb::OP_D, keep_del = !del || qmin <= 0 || del_kept(q, m, strand, li, qmin);
      for (int64_t t = p.lane(); t < ln; t += P::W)
        out[lo + t] = del ? (keep_del ? make_key(contig, lr + t, CODE_DEL) : DROPPED)
                          : qmin <= 0 || mmb::oriented_qual(q, m, strand, li + t) >= qmin ? make_key(contig, lr + t, oriented_code(q, m, strand, li + t)) : DROPPED;
    }
  }
  return at;
}

// the same without a floor, of a read source without qualities
template <class P, class Q> MM_HD int64_t emit_job(P& p, const Q& q, int64_t m, int32_t strand, int64_t contig, int64_t first, const uint32_t* ops, int64_t n_ops, uint64_t* out) {
  return emit_job_q(p, mmb::NoQual<Q>{q}, m, strand, contig, first, ops, n_ops, 0, out);
}

// first index of the ascending a[0, n) with a[i] >= x (upper: a[i] > x)
MM_HD int64_t bound(const uint64_t* a, int64_t n, uint64_t x, bool upper) {
  int64_t lo = 0, hi = n;
  while (lo < hi) { const int64_t mid = lo + (hi - lo) / 2; if (upper ? a[mid] <= x : a[mid] < x) lo = mid + 1; else hi = mid; }
  return lo;
}
MM_HD uint64_t interval_key(int64_t contig, int64_t pos) { return (uint64_t)contig << 32 | (uint64_t)pos; }
// starts and ends: the interval keys of every alignment's first and last base, each ascending
MM_HD int64_t depth_at(const uint64_t* starts, const uint64_t* ends, int64_t n_iv, int64_t contig, int64_t pos) {
  const uint64_t x = interval_key(contig, pos);
  return bound(starts, n_iv, x, true) - bound(ends, n_iv, x, false);
}
MM_HD bool site_kept(uint32_t count, int64_t depth, int64_t min_count, double min_frac) {
  return (int64_t)count >= min_count && (double)count >= min_frac * (double)depth;
}
// what interval i of the intervals sorted by start adds to its contig's covered positions: the part of [start, end] beyond prev_max, the largest
// end key of the intervals before it (has_prev: there is one).  Keys of another contig compare below or above as a whole.
MM_HD int64_t covered_gain(uint64_t start, uint64_t end, bool has_prev, uint64_t prev_max) {
  const uint64_t lo = has_prev && prev_max >= start ? prev_max + 1 : start;
  return end >= lo ? (int64_t)(end - lo + 1) : 0;
}

// the host's lane policy: one lane
struct HostLanes {
  static constexpr uint32_t W = 1;
  uint32_t lane() const { return 0; }
  int64_t scan_add(int64_t v, int64_t* total) const { *total = v; return 0; }
  uint64_t ballot(bool b) const { return b ? 1u : 0u; }
  int64_t pick(int64_t v, uint32_t) const { return v; }
};

}  // namespace mmp
