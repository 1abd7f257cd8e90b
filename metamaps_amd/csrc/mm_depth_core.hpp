// The depth profile of a run's primary alignments (mapDirectly --depth; DESIGN.md section 1, "Depth"): runs of equal depth, per-contig statistics and
// windows, written once for the kernels of mm_depth.hip and for the host (plain g++: tests/test_depth_core.cpp holds it to tests/depth_ref.py).  Interval
// keys, the binary search and depth_at are mm_pileup_core.hpp's.
//
//   inputs     n_contigs lengths len[c], 1 <= len < 2^29, n_contigs <= 2^29; n_iv intervals (c, first, last), 0 <= first <= last < len[c]; a window W >= 1;
//              0 to 8 strictly ascending thresholds T >= 1.  Nothing depends on the order of the intervals.
//   depth      of (c, p): the intervals on c with first <= p <= last (mm_pileup_finish's depth).  It changes only at the breakpoints c << 32 | first and
//              c << 32 | last + 1 (last + 1 <= len < 2^29: the key stays inside its contig), so everything below takes memory proportional to n_iv.
//   pieces     the breakpoints sorted and unique: u[0 .. m).  Piece j is [pos(u[j]), pos(u[j + 1])) at depth_at(u[j]), which is
//              (starts <= u[j]) - (ends < u[j]) over the sorted keys of every first and every last.  The last breakpoint of a contig is an end, so its depth
//              is 0: a piece of depth >= 1 always has its successor on the same contig.
//   runs       the maximal [start, end) of equal depth >= 1 inside one contig, ordered by contig, then start.  A piece heads a run where its depth is >= 1
//              and the piece before it is not on the same contig at the same depth (neighbouring pieces of a contig abut: [0,4] and [5,9] at depth 1 are the
//              run [0, 10), and a start on another's last + 1 changes nothing); it ends one where the next piece's depth differs.  Zero depth is not listed.
//   contigs    for every contig with an interval, ascending: alignments, covered (positions of depth >= 1), sumDepth (the three of PREFIX.pileup.contigs),
//              medianDepth (the depth at rank (len - 1) / 2, 0-based, of the contig's len depths sorted ascending, zeros included), maxDepth, and per
//              threshold ge[t], the positions of depth >= T[t].  All from prefix sums over the runs in start order (lengths, length * depth) and in
//              (contig, depth) order (lengths): the median is the first run, by depth, whose cumulated length passes rank - (len - covered).
//   windows    for every such contig all windows [kW, min((k + 1)W, len)), k < ceil(len / W), each with sum (of the depths) and covered: the runs that
//              meet the window from two binary searches, the prefix sums between them, less the parts of the first and the last run outside the window.
//              win_off[j] is the first window of the j-th listed contig.  2^31 - 1 windows at most.
//   widths     a depth is 32-bit (n_iv < 2^31), positions and all sums are 64-bit (a sum is at most n_iv * 2^29 < 2^60).
//
// Bounds: every function reads the arrays it is given inside the counts it is given; the run arrays hold n_runs entries and their prefix sums n_runs + 1.
#pragma once
#include "mm_pileup_core.hpp"

namespace mmdp {

// a contig's counters, in the order of mm_depth_fetch_contigs; ge[t] follows at STATS + t
enum Stat { ALIGNMENTS = 0, COVERED, SUM_DEPTH, MEDIAN_DEPTH, MAX_DEPTH, STATS };
constexpr int MAX_THRESHOLDS = 8;
constexpr int64_t MAX_LEN = ((int64_t)1 << 29) - 1, MAX_CONTIGS = (int64_t)1 << 29, MAX_WINDOWS = ((int64_t)1 << 31) - 1;
constexpr uint64_t POS_MASK = 0xFFFFFFFFull;

struct Thresholds { int32_t n; int64_t t[MAX_THRESHOLDS]; };

MM_HD bool length_ok(int64_t len) { return len >= 1 && len <= MAX_LEN; }
MM_HD bool interval_ok(int64_t contig, int64_t first, int64_t last, int64_t n_contigs, const int64_t* len) {
  return contig >= 0 && contig < n_contigs && first >= 0 && first <= last && last < len[contig];
}
MM_HD bool thresholds_ok(int32_t n, const int64_t* t) {
  if (n < 0 || n > MAX_THRESHOLDS) return false;
  for (int32_t k = 0; k < n; ++k) if (t[k] < 1 || (k > 0 && t[k] <= t[k - 1])) return false;
  return true;
}
MM_HD int64_t window_count(int64_t len, int64_t window) { return (len - 1) / window + 1; }   // (no sum of the two: W may be any int64)

MM_HD int64_t key_contig(uint64_t key) { return (int64_t)(key >> 32); }
MM_HD int64_t key_pos(uint64_t key) { return (int64_t)(key & POS_MASK); }
// the breakpoint behind an interval whose last base has the key `end_key`
MM_HD uint64_t end_break(uint64_t end_key) { return end_key + 1; }
// starts, ends: the interval keys of every first and every last base, each ascending; the depth of the piece that starts at the breakpoint `key`
MM_HD uint32_t piece_depth(const uint64_t* starts, const uint64_t* ends, int64_t n_iv, uint64_t key) {
  return (uint32_t)(mmp::bound(starts, n_iv, key, true) - mmp::bound(ends, n_iv, key, false));
}
MM_HD bool run_head(bool has_prev, uint64_t prev_key, uint32_t prev_depth, uint64_t key, uint32_t depth) {
  return depth > 0 && !(has_prev && key_contig(prev_key) == key_contig(key) && prev_depth == depth);
}
MM_HD bool run_tail(uint32_t depth, bool has_next, uint32_t next_depth) { return depth > 0 && (!has_next || next_depth != depth); }

// The runs in start order: rstart[r] = contig << 32 | start, rend[r] = contig << 32 | end (both ascending), rdepth[r]; plen and psum the exclusive prefix
// sums of end - start and of (end - start) * depth, n_runs + 1 entries each.
struct Runs { int64_t n; const uint64_t* rstart; const uint64_t* rend; const uint32_t* rdepth; const uint64_t* plen; const uint64_t* psum; };
// The runs in (contig, depth) order: dkey[r] = contig << 32 | depth ascending, dlen the exclusive prefix sums of their lengths (n_runs + 1 entries).  A
// contig's runs hold the same places [s, e) in both orders.
struct RunsByDepth { const uint64_t* dkey; const uint64_t* dlen; };

// out[STATS + T.n]: the counters of contig c of length len, which has at least one run; starts: the intervals' start keys, ascending
MM_HD void contig_stats(int64_t c, int64_t len, const uint64_t* starts, int64_t n_iv, const Runs& R, const RunsByDepth& D, const Thresholds& T, int64_t* out) {
  const uint64_t lo = mmp::interval_key(c, 0), hi = mmp::interval_key(c + 1, 0);
  const int64_t s = mmp::bound(R.rstart, R.n, lo, false), e = mmp::bound(R.rstart, R.n, hi, false);
  const int64_t covered = (int64_t)(R.plen[e] - R.plen[s]);
  out[ALIGNMENTS] = mmp::bound(starts, n_iv, hi, false) - mmp::bound(starts, n_iv, lo, false);
  out[COVERED] = covered;
  out[SUM_DEPTH] = (int64_t)(R.psum[e] - R.psum[s]);
  const int64_t rank = (len - 1) / 2, zeros = len - covered;
  int64_t median = 0;
  if (rank >= zeros && e > s) {                                   // the first run, by depth, whose cumulated length passes rank - zeros
    const int64_t i = s + mmp::bound(D.dlen + s + 1, e - s, D.dlen[s] + (uint64_t)(rank - zeros), true);
    median = (int64_t)(D.dkey[i < e ? i : e - 1] & POS_MASK);
  }
  out[MEDIAN_DEPTH] = median;
  out[MAX_DEPTH] = e > s ? (int64_t)(D.dkey[e - 1] & POS_MASK) : 0;
  for (int32_t t = 0; t < T.n; ++t) {
    int64_t ge = 0;
    if (T.t[t] <= (int64_t)POS_MASK) {                            // (a depth is 32-bit: nothing reaches a larger threshold)
      int64_t i = mmp::bound(D.dkey, R.n, lo | (uint64_t)T.t[t], false);
      i = i < s ? s : i > e ? e : i;
      ge = (int64_t)(D.dlen[e] - D.dlen[i]);
    }
    out[STATS + t] = ge;
  }
}

// the window [a, b) of contig c, 0 <= a < b <= len: the sum of its depths and its positions of depth >= 1
MM_HD void window_sums(int64_t c, int64_t a, int64_t b, const Runs& R, int64_t* sum, int64_t* covered) {
  const int64_t r0 = mmp::bound(R.rend, R.n, mmp::interval_key(c, a), true);    // the first run that ends behind a
  const int64_t r1 = mmp::bound(R.rstart, R.n, mmp::interval_key(c, b), false);  // the first run that starts at b or later
  *sum = 0; *covered = 0;
  if (r0 >= r1) return;
  uint64_t s = R.psum[r1] - R.psum[r0], n = R.plen[r1] - R.plen[r0];
  const int64_t head = a - key_pos(R.rstart[r0]), tail = key_pos(R.rend[r1 - 1]) - b;   // what the first and the last run hold outside the window
  if (head > 0) { s -= (uint64_t)head * R.rdepth[r0]; n -= (uint64_t)head; }
  if (tail > 0) { s -= (uint64_t)tail * R.rdepth[r1 - 1]; n -= (uint64_t)tail; }
  *sum = (int64_t)s; *covered = (int64_t)n;
}
// window k < window_count(len, window) of a contig: [a, b)
MM_HD void window_span(int64_t len, int64_t window, int64_t k, int64_t* a, int64_t* b) { *a = k * window; *b = len - *a <= window ? len : *a + window; }
// the listed contig of window w: win_off[0 .. n_listed] ascending from 0
MM_HD int64_t window_contig(const uint64_t* win_off, int64_t n_listed, int64_t w) { return mmp::bound(win_off, n_listed + 1, (uint64_t)w, true) - 1; }

}  // namespace mmdp
