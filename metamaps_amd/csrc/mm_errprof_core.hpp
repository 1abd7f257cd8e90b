// The error profile of a run's primary alignments (mapDirectly --error-profile; DESIGN.md section 1, "Error profile"): what every alignment says about the
// reads and about the distance between the sample and the reference, written once for the kernels of mm_errprof.hip (one wavefront per job at a time) and
// for the host (plain g++: tests/test_errprof_core.cpp holds it to tests/errprof_ref.py).
//
//   runs      an aligned job has first, strand, contig, read and the runs mm_alignment_fetch gives (len << 4 | op; I 1, D 2, = 7, X 8), those of the
//             oriented read Q (the reverse complement for strand -1) along the forward contig R.  m is the read's length, q(i) = mmb::oriented_qual
//             (0xFF: none), code = mmp::base_code (A 0 C 1 G 2 T 3, else N 4), comp = mmp::complement.
//   walk      r = first, i = 0:
//               = or X at (r, i)   counted as the sequencer saw it: truth a = code(R[r]) (comp of it for strand -1), observed b = code of the STORED read byte
//                                  of that base (comp(code(Q[i])) for -1); SUB[a * 5 + b] += 1; QUAL[cls][row(q(i))] += 1, cls 0 for =, 1 for X
//               I of n at (r, i)   QUAL[2][row(q(i + t))] += 1 for t < n; INDEL[0][hp][min(n, 64) - 1] += 1 with hp = 1 iff the n oriented bases are one
//                                  letter b of A C G T and (r >= 1 and R[r - 1] == b, or r < the contig's length and R[r] == b)
//               D of n at r        INDEL[1][hp][min(n, 64) - 1] += 1 with hp = 1 iff R[r .. r + n) is one letter b of A C G T and (r >= 1 and R[r - 1] == b,
//                                  or r + n < the contig's length and R[r + n] == b)
//             row(q) = q for 0..93, 94 for "no quality".
//   columns   per job eq, x, insRuns, insBases, delRuns, delBases; all zero for a job that is not used.
//   key       contig << 32 | ppm with ppm = floor(10^6 * eq / (eq + x + insBases + delBases)) in 64-bit integers (the denominator is >= 1 once the rules
//             hold and the read is not empty; a job without columns has ppm 0); NO_KEY for a job that is not used.
//   counters  COUNTERS = 25 + 2 * 2 * 64 + 3 * 95 = 566 in the order SUB, INDEL[kind][hp][bin], QUAL[cls][row].  They add across jobs, calls, batches and
//             devices, so nothing depends on batch size, devices or order.
//   checks    mmp::count_job's (mm_bam_encode's rules 1, 2 (the strand), 4, 5 and 6): after them every read index of the walk is inside the read, every
//             r of a column inside the contig, and r of an indel in [0, the contig's length].
//   finish    the (key, columns) of a query file's contributing alignments, sorted by key: per contig the alignments, the six sums and of its ppm values
//             v[0 .. n) ascending min = v[0], q1 = v[(n - 1) / 4], median = v[(n - 1) / 2], q3 = v[3 (n - 1) / 4], max = v[n - 1] (rank_of).
//
// The walk is defined over tiles of P::W runs, one run per lane (mm_pileup_core.hpp's lane policy: lane, scan_add, ballot, pick); a lane walks its own run
// of up to LONG_RUN bases, a longer run is walked by all lanes of the tile.  T takes the increments: t.add(index) adds 1 to counter `index`.
// Q gives q.byte(i) and q.qual(i) of the stored read, R gives ref.byte(p) of the contig.
//
// Bounds: walk_job reads ops[0, n_ops), q.byte / q.qual (0 .. m - 1), ref.byte(0 .. contig_len - 1) and adds to indexes below COUNTERS.
#pragma once
#include "mm_pileup_core.hpp"

namespace mmep {

constexpr uint32_t SUB = 0, N_SUB = 25, BINS = 64, INDEL = SUB + N_SUB, N_INDEL = 2 * 2 * BINS, QROWS = 95, QUAL = INDEL + N_INDEL, N_QUAL = 3 * QROWS;
constexpr uint32_t COUNTERS = QUAL + N_QUAL;                      // 566
constexpr int COLS = 6;
enum Col : int { EQ = 0, X = 1, INS_RUNS = 2, INS_BASES = 3, DEL_RUNS = 4, DEL_BASES = 5 };
constexpr int STATS = 12;                                         // of a contig's row: alignments, the six sums, min, q1, median, q3, max of ppm
enum Stat : int { ALIGNMENTS = 0, SUM0 = 1, PPM_MIN = 7, PPM_Q1 = 8, PPM_MEDIAN = 9, PPM_Q3 = 10, PPM_MAX = 11 };
constexpr uint64_t NO_KEY = ~0ull;
constexpr int64_t LONG_RUN = 64;                                  // a longer run is walked by all lanes of the tile
constexpr int64_t MAX_CONTIGS = (int64_t)1 << 31;

MM_HD uint32_t qual_row(uint8_t q) { return q <= 93 ? q : QROWS - 1; }
MM_HD uint32_t sub_at(uint32_t truth, uint32_t seen) { return SUB + truth * 5 + seen; }
MM_HD uint32_t indel_at(uint32_t kind, bool hp, int64_t n) { return INDEL + (kind * 2 + (hp ? 1u : 0u)) * BINS + (uint32_t)((n < (int64_t)BINS ? n : (int64_t)BINS) - 1); }
MM_HD uint32_t qual_at(uint32_t cls, uint8_t q) { return QUAL + cls * QROWS + qual_row(q); }

MM_HD uint64_t ident_key(int64_t contig, const int64_t* c) {
  const int64_t den = c[EQ] + c[X] + c[INS_BASES] + c[DEL_BASES];
  const uint64_t ppm = den > 0 ? (uint64_t)(1000000 * c[EQ] / den) : 0;
  return (uint64_t)contig << 32 | ppm;
}
MM_HD int64_t key_contig(uint64_t key) { return (int64_t)(key >> 32); }
MM_HD int64_t key_ppm(uint64_t key) { return (int64_t)(key & 0xFFFFFFFFull); }
// the rank of statistic s (PPM_MIN .. PPM_MAX) among n >= 1 ascending values
MM_HD int64_t rank_of(int s, int64_t n) {
  return s == PPM_MIN ? 0 : s == PPM_Q1 ? (n - 1) / 4 : s == PPM_MEDIAN ? (n - 1) / 2 : s == PPM_Q3 ? 3 * (n - 1) / 4 : n - 1;
}

// bases t0, t0 + step, ... of a run of n at (r, i): the columns of an = or X run and the qualities of an I run are counted; returns whether every one of
// these bases of an I run (reference bytes of a D run) has code b
template <class Q, class R, class T> MM_HD bool run_part(const Q& q, const R& ref, int64_t m, int32_t strand, uint32_t op, int64_t r, int64_t i, int64_t n, int64_t t0, int64_t step,
                                                         uint32_t b, T& t) {
  bool same = true;
  if (op == mmb::OP_D) {
    for (int64_t k = t0; k < n; k += step) same = same && mmp::base_code(ref.byte(r + k)) == b;
    return same;
  }
  for (int64_t k = t0; k < n; k += step) {
    const uint32_t seen = mmp::base_code(q.byte(strand < 0 ? m - 1 - (i + k) : i + k));   // the stored byte: what the sequencer wrote
    const uint8_t ql = mmb::oriented_qual(q, m, strand, i + k);
    if (op == mmb::OP_I) {
      same = same && (strand < 0 ? mmp::complement(seen) : seen) == b;
      t.add(qual_at(2, ql));
    } else {
      const uint32_t rc = mmp::base_code(ref.byte(r + k));
      t.add(sub_at(strand < 0 ? mmp::complement(rc) : rc, seen));
      t.add(qual_at(op == mmb::OP_X ? 1 : 0, ql));
    }
  }
  return same;
}
// the letter an indel run at (r, i) would have to repeat: its first oriented base (I) or its first reference byte (D)
template <class Q, class R> MM_HD uint32_t indel_letter(const Q& q, const R& ref, int64_t m, int32_t strand, uint32_t op, int64_t r, int64_t i) {
  return op == mmb::OP_D ? mmp::base_code(ref.byte(r)) : mmp::oriented_code(q, m, strand, i);
}
// hp of an indel run of n whose bases are all the letter b (same): a neighbour of the run on the reference is b too
template <class R> MM_HD bool indel_hp(const R& ref, int64_t contig_len, uint32_t op, int64_t r, int64_t n, uint32_t b, bool same) {
  if (!same || b >= 4) return false;
  const int64_t behind = op == mmb::OP_D ? r + n : r;
  return (r >= 1 && mmp::base_code(ref.byte(r - 1)) == b) || (behind < contig_len && mmp::base_code(ref.byte(behind)) == b);
}

// a job whose checks have passed: its increments to t, its six columns to cols (the same in every lane)
template <class P, class Q, class R, class T> MM_HD void walk_job(P& p, const Q& q, const R& ref, int64_t m, int32_t strand, int64_t first, int64_t contig_len, const uint32_t* ops,
                                                                  int64_t n_ops, T& t, int64_t* cols) {
  int64_t rsum = 0, isum = 0;                                     // the running values: the same in every lane
  int64_t mine[COLS] = {0, 0, 0, 0, 0, 0};                        // this lane's runs
  for (int64_t base = 0; base < n_ops; base += P::W) {
    const mmp::Run x = mmp::run_of(ops, base + p.lane(), n_ops);
    int64_t tot;
    const int64_t r = first + rsum + p.scan_add(x.good && x.op != mmb::OP_I ? x.len : 0, &tot); rsum += tot;
    const int64_t i = isum + p.scan_add(x.good && x.op != mmb::OP_D ? x.len : 0, &tot); isum += tot;
    const bool indel = x.good && (x.op == mmb::OP_I || x.op == mmb::OP_D);
    if (x.good) {
      if (x.op == mmb::OP_EQ) mine[EQ] += x.len;
      else if (x.op == mmb::OP_X) mine[X] += x.len;
      else if (x.op == mmb::OP_I) { mine[INS_RUNS] += 1; mine[INS_BASES] += x.len; }
      else { mine[DEL_RUNS] += 1; mine[DEL_BASES] += x.len; }
    }
    const bool wide = x.good && x.len > LONG_RUN;
    const uint32_t b = indel ? indel_letter(q, ref, m, strand, x.op, r, i) : 0;
    if (x.good && !wide) {                                         // a short run: its own lane walks it
      const bool same = run_part(q, ref, m, strand, x.op, r, i, x.len, 0, 1, b, t);
      if (indel) t.add(indel_at(x.op == mmb::OP_D ? 1 : 0, indel_hp(ref, contig_len, x.op, r, x.len, b, same), x.len));
    }
    for (uint64_t left = p.ballot(wide); left; left &= left - 1) {   // the long runs of the tile, one after the other, by all lanes
      uint32_t l = 0;
      while (!(left >> l & 1)) ++l;
      const int64_t lr = p.pick(r, l), li = p.pick(i, l), ln = p.pick(x.len, l);
      const uint32_t lop = (uint32_t)p.pick((int64_t)x.op, l), lb = (uint32_t)p.pick((int64_t)b, l);
      const bool same = p.ballot(!run_part(q, ref, m, strand, lop, lr, li, ln, (int64_t)p.lane(), (int64_t)P::W, lb, t)) == 0;
      if ((lop == mmb::OP_I || lop == mmb::OP_D) && p.lane() == 0) t.add(indel_at(lop == mmb::OP_D ? 1 : 0, indel_hp(ref, contig_len, lop, lr, ln, lb, same), ln));
    }
  }
  for (int k = 0; k < COLS; ++k) (void)p.scan_add(mine[k], &cols[k]);
}

// the host's sink: 64-bit counters
struct HostCounters {
  uint64_t* c;
  void add(uint32_t index) { c[index] += 1; }
};

}  // namespace mmep
