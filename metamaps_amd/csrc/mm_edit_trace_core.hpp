// Base-level alignments of mappings (mapDirectly --paf; DESIGN.md section 1, "Alignments"): the storing pass of Myers' block recurrence and the walk
// back through what it stored, one text for the host build and for the kernel of mm_edit.hip.  The definition of the alignment is mm_edit_core.hpp's;
// d, a, b, the blocks, the 64-lane schedule and the strings are mm_edit_bv_core.hpp's, whose two passes stay as they are.
//   reversed  E[i][j] of the definition is the anchored table D of reverse(Q) against reverse(T), T = window[a, b): E[i][j] = D[m - i][n - j].  The
//             walk from (0, 0) to (m, n) through E is the walk from D's last cell (m, n) back to its origin, and its operations come out in forward
//             order, the alignment's first run first.  n = b - a and D[m][n] = d are known on entry.
//   pass 3    the anchored recurrence once more (hin0 = +1, as pass 2), on n columns.  For every cell the walk's choice is two bits, and the pass
//             stores those instead of deltas: with Eq the column's match bits, D0 = Xh | Mv the cells whose diagonal delta is 0 (Myers' D0; Mv the
//             one before the column) and Pv the column's new vertical +1 bits
//               w0 = Eq | ~D0                 the step is diagonal: = where Eq, else X (D[i-1][j-1] + 1 == D[i][j])
//               w1 = w0 ? Eq : Pv             diagonal: which of the two; else I where the cell above is one less, else D
//             2 words per block and column: no running score, no popcount and no string access in the walk.
//   layout    word p of block k of lane l at step t (column t - l) lies at ((t 2B + 2k + p) 64 + l): one store instruction of the wavefront writes
//             256 consecutive bytes.  A job's scratch is bv_trace_words(m, n) = (n + 63) 64 2B words.
//   walk      every lane steps the same walk.  Where it needs a cell outside what is loaded, lane x fetches the two words of column c - x for the
//             block the walk is in and for the one above, c the walk's column: a strip of 64 columns by two blocks; the steps inside it take their
//             words by pick (a __shfl on the device).  At most m + n steps; row 0 goes left (D), column 0 goes up (I).
//   runs      len << 4 | op as BAM has them (I 1, D 2, = 7, X 8) into the job's slot of 2 d + 1 words (d edits separate at most d + 1 runs of =).
// The lanes G are mm_edit_bv_core.hpp's with sync() added: the stores of pass 3 are visible to the other lanes behind it.
//
// Compiles for host (tests/test_edit_trace_core.cpp via g++) and, under hipcc, for the device.
#pragma once
#include "mm_edit_bv_core.hpp"

namespace mm {

constexpr uint32_t CIG_I = 1, CIG_D = 2, CIG_EQ = 7, CIG_X = 8;

MM_HD int64_t bv_trace_words(int32_t m, int32_t n) { return m > 0 && n > 0 ? ((int64_t)n + BV_LANES - 1) * BV_LANES * 2 * bv_per_lane(m) : 0; }
MM_HD int64_t bv_trace_slot(int32_t d) { return 2 * (int64_t)d + 1; }
MM_HD int64_t bv_trace_at(int32_t B, int32_t t, int32_t k, int lane) { return ((int64_t)t * (2 * B) + 2 * k) * BV_LANES + lane; }   // w0; w1 lies BV_LANES further

// bv_block that also gives the walk's two words of the block's cells in this column
MM_HD int bv_block_trace(uint32_t Eq, uint32_t& Pv, uint32_t& Mv, int hin, uint32_t top, uint32_t* w0, uint32_t* w1) {
  const uint32_t neg = hin < 0 ? 1u : 0u, pos = hin > 0 ? 1u : 0u, eq = Eq;
  const uint32_t Xv = Eq | Mv;
  Eq |= neg;
  const uint32_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
  const uint32_t diag = eq | ~(Xh | Mv);
  uint32_t Ph = Mv | ~(Xh | Pv), Mh = Pv & Xh;
  const int hout = (Ph & top) ? 1 : (Mh & top) ? -1 : 0;
  Ph = (Ph << 1) | pos; Mh = (Mh << 1) | neg;
  Pv = Mh | ~(Xv | Ph); Mv = Ph & Xv;
  *w0 = diag; *w1 = (diag & eq) | (~diag & Pv);
  return hout;
}
MM_HD uint32_t bv_trace_op(uint32_t w0, uint32_t w1, int bit) {
  const uint32_t p0 = (w0 >> bit) & 1u, p1 = (w1 >> bit) & 1u;
  return p0 ? (p1 ? CIG_EQ : CIG_X) : (p1 ? CIG_I : CIG_D);
}

// the runs of a walk: push every operation, then flush; count may pass cap (it never does: 2 d + 1), the words behind cap are not written
struct BvRuns {
  uint32_t* slot; int64_t cap; bool writes; int64_t count; uint32_t op, len;
  MM_HD void flush() { if (len) { if (writes && count < cap) slot[count] = len << 4 | op; ++count; } len = 0; }
  MM_HD void push(uint32_t o) { if (o != op) { flush(); op = o; } ++len; }
};

// step t of one lane in pass 3: bv_lane_step without the score, with the stores (scr: the job's scratch)
template <int BT> MM_HD uint32_t bv_lane_step_trace(const BvPass& P, int lane, int32_t t, uint32_t in, const uint32_t* peq, BvLane<BT>& L, uint32_t* scr) {
  const int32_t j = bv_column(t, lane);
  if (j < 0 || j >= P.n || L.nb == 0) return in;
  const uint32_t sym = bv_msg_sym(in), hit = sym < 4 ? ~0u : 0u;
  const uint32_t* w = peq + (size_t)(sym & 3u) * BV_LANES;
  uint32_t* out = scr + bv_trace_at(P.B, t, 0, lane);
  int h = bv_msg_h(in);
MM_BV_UNROLL
  for (int k = 0; k < BT; ++k)
    if (k < L.nb) {
      uint32_t w0, w1;
      h = bv_block_trace(w[(size_t)(4 * k) * BV_LANES] & hit, L.pv[k], L.mv[k], h, lane == P.last_lane && k == L.nb - 1 ? P.top : 1u << (BV_W - 1), &w0, &w1);
      out[(size_t)(2 * k) * BV_LANES] = w0; out[(size_t)(2 * k + 1) * BV_LANES] = w1;
    }
  return bv_msg(sym, h);
}

// pass 3 on the lanes G (P anchored, q and r reversed): bv_run_pass's loop with the storing step
template <int BT, class G, class Q, class R> MM_HD void bv_trace_pass(const G& g, const BvPass& P, const Q& q, const R& r, uint32_t* peq, uint32_t* scr) {
  BvLane<BT> L[G::HELD];
  uint32_t out[G::HELD], in[G::HELD], text[G::HELD];
  for (int h = 0; h < G::HELD; ++h) { bv_lane_init<BT>(P, g.lane(h), q, peq + g.lane(h), L[h]); out[h] = 0; text[h] = BV_SYM_NONE; }
  const int32_t steps = P.blocks ? bv_steps(P) : 0;
  for (int32_t t = 0; t < steps; ++t) {
    if ((t & (BV_LANES - 1)) == 0)
      for (int h = 0; h < G::HELD; ++h) { const int32_t j = t + g.lane(h); text[h] = j < P.n ? r.at(j) : (uint32_t)BV_SYM_NONE; }
    g.up(out, in);
    const uint32_t s0 = g.pick(text, t & (BV_LANES - 1));
    for (int h = 0; h < G::HELD; ++h) if (g.lane(h) == 0) in[h] = bv_msg(s0, P.hin0);
    for (int h = 0; h < G::HELD; ++h) out[h] = bv_lane_step_trace<BT>(P, g.lane(h), t, in[h], peq + g.lane(h), L[h], scr);
  }
}

// the walk through a job's scratch; the runs go to slot (lane 0 writes), at most cap of them; returns their number
template <class G> MM_HD int64_t bv_trace_walk(const G& g, const BvPass& P, const uint32_t* scr, uint32_t* slot, int64_t cap) {
  uint32_t a0[G::HELD], a1[G::HELD], b0[G::HELD], b1[G::HELD];    // the strip: lane x has column ld_col - x of block ld_blk (a) and ld_blk - 1 (b)
  for (int h = 0; h < G::HELD; ++h) { a0[h] = a1[h] = b0[h] = b1[h] = 0; }
  int32_t ld_blk = -1, ld_col = -1;
  bool lane0 = false;
  for (int h = 0; h < G::HELD; ++h) lane0 = lane0 || g.lane(h) == 0;
  BvRuns runs{slot, cap, lane0, 0, 0, 0};
  int32_t i = P.m, j = P.n;
  const int64_t most = (int64_t)P.m + P.n;
  for (int64_t s = 0; s < most && (i > 0 || j > 0); ++s) {
    uint32_t op;
    if (i == 0) op = CIG_D;
    else if (j == 0) op = CIG_I;
    else {
      const int32_t row = i - 1, col = j - 1, blk = row / BV_W;
      if (ld_blk < 0 || blk > ld_blk || blk < ld_blk - 1 || col > ld_col || col <= ld_col - BV_LANES) {
        ld_blk = blk; ld_col = col;
        for (int h = 0; h < G::HELD; ++h) {
          const int32_t c = col - g.lane(h);
          if (c < 0) continue;
          const int32_t la = blk / P.B;
          const uint32_t* w = scr + bv_trace_at(P.B, c + la, blk - la * P.B, la);
          a0[h] = w[0]; a1[h] = w[BV_LANES];
          if (blk > 0) {
            const int32_t lb = (blk - 1) / P.B;
            w = scr + bv_trace_at(P.B, c + lb, blk - 1 - lb * P.B, lb);
            b0[h] = w[0]; b1[h] = w[BV_LANES];
          }
        }
      }
      const int x = ld_col - col;
      const bool lower = blk == ld_blk;
      op = bv_trace_op(g.pick(lower ? a0 : b0, x), g.pick(lower ? a1 : b1, x), row & (BV_W - 1));
    }
    runs.push(op);
    if (op != CIG_D) --i;
    if (op != CIG_I) --j;
  }
  runs.flush();
  return runs.count;
}

// the runs of a job whose d, a, b are known (d >= 0): the stored read [q_org, q_org + m) of qs on `strand` against rs's [r_org, r_org + n), which
// is window[a, b).  peq: bv_peq_words words; scr: bv_trace_words(m, n) words; slot: bv_trace_slot(d) words.  Returns the number of runs.
template <int BT, class G, class QS, class RS>
MM_HD int64_t bv_trace(const G& g, const QS& qs, int64_t q_org, int32_t m, int strand, const RS& rs, int64_t r_org, int32_t n, int32_t d, uint32_t* peq, uint32_t* scr, uint32_t* slot) {
  if (m <= 0) return 0;
  const BvPass P = bv_pass(m, n, true);
  bv_trace_pass<BT>(g, P, BvString<QS>{qs, q_org, m, strand < 0, true}, BvString<RS>{rs, r_org, n, false, true}, peq, scr);
  g.sync();
  return bv_trace_walk(g, P, scr, slot, bv_trace_slot(d));
}

}  // namespace mm

// ---- the whole definition on one host thread, both forms (the tests' host build) ----
#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>

namespace mm {

struct BvTraceHostLanes : BvHostLanes { void sync() const {} };

struct TraceHostResult { int32_t dist; int64_t begin, end, n_runs; std::vector<uint32_t> runs; };   // n_runs: what the walk counted (runs.size() unless it passed the slot)

// the serial form: every column's words of every block (2 nb words per column), then the walk cell by cell
inline int64_t bv_trace_serial(const BvString<BvBytes>& q, const BvString<BvBytes>& r, int32_t m, int32_t n, uint32_t* slot, int64_t cap) {
  const int32_t nb = bv_blocks(m);
  if (m <= 0) return 0;
  std::vector<uint32_t> peq((size_t)4 * nb, 0u), pv((size_t)nb, ~0u), mv((size_t)nb, 0u), w((size_t)2 * nb * (size_t)n + 2);
  for (int32_t i = 0; i < m; ++i) { const uint32_t y = q.at(i); if (y < 4) peq[4 * (size_t)(i / BV_W) + y] |= 1u << (i % BV_W); }
  for (int32_t j = 0; j < n; ++j) {
    const uint32_t y = r.at(j);
    int h = 1;
    for (int32_t k = 0; k < nb; ++k) {
      uint32_t* o = &w[((size_t)j * nb + k) * 2];
      h = bv_block_trace(y < 4 ? peq[4 * (size_t)k + y] : 0u, pv[k], mv[k], h, k == nb - 1 ? 1u << ((m - 1) & (BV_W - 1)) : 1u << (BV_W - 1), o, o + 1);
    }
  }
  BvRuns runs{slot, cap, true, 0, 0, 0};
  int32_t i = m, j = n;
  while (i > 0 || j > 0) {
    uint32_t op = i == 0 ? CIG_D : CIG_I;
    if (i > 0 && j > 0) { const uint32_t* o = &w[((size_t)(j - 1) * nb + (i - 1) / BV_W) * 2]; op = bv_trace_op(o[0], o[1], (i - 1) & (BV_W - 1)); }
    runs.push(op);
    if (op != CIG_D) --i;
    if (op != CIG_I) --j;
  }
  runs.flush();
  return runs.count;
}

// read: L bytes as stored; window: the n bytes of contig[ws, we).  d, a, b as bv_infix_host gives them, and the runs
inline TraceHostResult bv_trace_host(const char* read, int64_t L, int strand, const char* window, int64_t n, int32_t max_dist, bool pipeline) {
  const EditHostResult e = bv_infix_host(read, L, strand, window, n, max_dist, pipeline);
  TraceHostResult res{e.dist, e.begin, e.end, 0, {}};
  if (e.dist < 0 || L <= 0) return res;
  const int32_t m = (int32_t)L, nt = (int32_t)(e.end - e.begin);
  const BvBytes qs{read}, rs{window};
  res.runs.assign((size_t)bv_trace_slot(e.dist), 0u);
  int64_t count = 0;
  if (pipeline) {
    std::vector<uint32_t> peq((size_t)bv_peq_words(bv_per_lane(m)) + 1), scr((size_t)bv_trace_words(m, nt) + 1);
    const BvTraceHostLanes g;
    uint32_t* slot = res.runs.data();
    switch (bv_class(bv_per_lane(m))) {
      case 1: count = bv_trace<1>(g, qs, 0, m, strand, rs, e.begin, nt, e.dist, peq.data(), scr.data(), slot); break;
      case 2: count = bv_trace<2>(g, qs, 0, m, strand, rs, e.begin, nt, e.dist, peq.data(), scr.data(), slot); break;
      case 4: count = bv_trace<4>(g, qs, 0, m, strand, rs, e.begin, nt, e.dist, peq.data(), scr.data(), slot); break;
      case 8: count = bv_trace<8>(g, qs, 0, m, strand, rs, e.begin, nt, e.dist, peq.data(), scr.data(), slot); break;
      case 16: count = bv_trace<16>(g, qs, 0, m, strand, rs, e.begin, nt, e.dist, peq.data(), scr.data(), slot); break;
      default: count = bv_trace<32>(g, qs, 0, m, strand, rs, e.begin, nt, e.dist, peq.data(), scr.data(), slot); break;
    }
  } else {
    count = bv_trace_serial(BvString<BvBytes>{qs, 0, m, strand < 0, true}, BvString<BvBytes>{rs, e.begin, nt, false, true}, m, nt, res.runs.data(), bv_trace_slot(e.dist));
  }
  res.n_runs = count;
  res.runs.resize((size_t)(count < bv_trace_slot(e.dist) ? count : bv_trace_slot(e.dist)));
  return res;
}

}  // namespace mm
#endif

// ---- the launches of a batch (host code, also where the kernels are compiled): job i (read length m[i], dist[i] < 0: not aligned, nothing to trace) gets its place in the scratch of its launch and
// its slot; the jobs [cut[c], cut[c + 1]) are launch c, whose scratch fits budget_words.  A launch holds one job at least, so the budget is in
// effect raised to the largest job; no result depends on it.
#include <vector>

namespace mm {

struct TracePlan { std::vector<int64_t> scr_off, slot_off, cut; int64_t scratch_words = 0, slot_words = 0; };
inline bool bv_trace_wanted(int32_t m, int32_t dist) { return dist >= 0 && m > 0 && m <= EDIT_MAX_READ; }
inline TracePlan bv_trace_plan(int64_t n, const int32_t* m, const int32_t* dist, const int32_t* a, const int32_t* b, int64_t budget_words, int64_t max_jobs) {
  TracePlan P;
  P.scr_off.assign((size_t)n, 0); P.slot_off.assign((size_t)n, 0); P.cut.push_back(0);
  int64_t cur = 0;
  for (int64_t i = 0; i < n; ++i) {
    const bool on = bv_trace_wanted(m[i], dist[i]);
    const int64_t w = on ? bv_trace_words(m[i], b[i] - a[i]) : 0;
    if (i > P.cut.back() && ((w > 0 && cur + w > budget_words) || i - P.cut.back() >= max_jobs)) { P.cut.push_back(i); cur = 0; }
    P.scr_off[(size_t)i] = cur; cur += w;
    if (cur > P.scratch_words) P.scratch_words = cur;
    P.slot_off[(size_t)i] = P.slot_words; P.slot_words += on ? bv_trace_slot(dist[i]) : 0;
  }
  P.cut.push_back(n);
  return P;
}

}  // namespace mm
