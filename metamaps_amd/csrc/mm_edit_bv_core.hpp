// Exact edit distances of mappings by Myers' bit-vector recurrence in its block form (Myers 1999, Hyyro 2003; what Edlib runs for this semi-global
// problem): one text for the host build and for the kernel of mm_edit.hip.  The definition of d, a and b, the window, cap and base rules and the
// checks on a job's arguments are mm_edit_core.hpp's and are not restated here ("Edit distances").
//   blocks    the read is cut into blocks of BV_W = 32 rows; Peq[blk][c] has bit i set where read base 32 blk + i is the letter c (a read base that
//             matches nothing is in no Peq, a window base that matches nothing has Eq = 0).  Every block starts with Pv = all ones, Mv = 0, and the
//             bottom-row score starts at m.
//   column    for every window column the blocks are taken top to bottom (bv_block); the horizontal delta hout of one block is the hin of the next,
//             the top block takes hin = 0 in pass 1 (the window's start is free) and +1 in pass 2 (anchored); after the last block score += hout
//   pass 1    d = the smallest bottom-row score (row[0] = m), b = the first column with it
//   pass 2    the same routine on reverse(Q) against reverse(R[0, b)): e' = the first column whose score is the minimum (it is d), a = b - e'
//   schedule  one wavefront is a systolic pipeline: lane l owns the B = ceil(blocks / 64) consecutive blocks from l B on (equal for all lanes of a
//             job; the lanes behind the last block own none), at step t it works on column t - l and takes hout, and the column's symbol with it in
//             the same word, from lane l - 1's previous step.  Steps run 0 .. n + 62; a lane whose column lies outside [0, n) does nothing.  Lane 0
//             takes the symbols from the window text, which all lanes fetch together, 64 columns every 64 steps.  The lane that owns the last block
//             keeps the score, its minimum and the first column of the minimum.
// Nothing in the control flow depends on the strings: every loop's trip count is known when it is entered (m, n, and b for pass 2).
// The lanes G hold HELD lanes per thread of execution: all 64 in plain loops on the host (BvHostLanes), one per thread on the device (mm_edit.hip:
// the neighbour's word comes by __shfl_up).  The per-lane step, the step-to-column mapping with its fill and drain and the driver are this one text.
// Pv / Mv live in the lane (registers on the device), hence the compile-time bound BT >= B: a power of two, one kernel per class (bv_class).
//
// Compiles for host (tests/test_edit_bv_core.cpp via g++) and, under hipcc, for the device.
#pragma once
#include "mm_edit_core.hpp"

#if defined(__HIPCC__)
#define MM_BV_UNROLL _Pragma("unroll")
#else
#define MM_BV_UNROLL
#endif

namespace mm {

constexpr int BV_W = 32;                                          // rows per block: gfx950 adds 32-bit integers in one instruction, 64-bit ones as a carry pair
constexpr int BV_LANES = 64;
constexpr int BV_MAX_B = EDIT_MAX_READ / BV_W / BV_LANES;         // 32 blocks per lane at the longest read
constexpr int BV_SYM_NONE = 4;                                    // edit_sym's "matches nothing"

MM_HD int32_t bv_blocks(int32_t m) { return (m + BV_W - 1) / BV_W; }
MM_HD int32_t bv_per_lane(int32_t m) { return (bv_blocks(m) + BV_LANES - 1) / BV_LANES; }
MM_HD int32_t bv_class(int32_t B) { int32_t c = 1; for (int r = 0; r < 5 && c < B; ++r) c <<= 1; return c; }   // 1 2 4 8 16 32
MM_HD int64_t bv_peq_words(int32_t B) { return (int64_t)4 * BV_LANES * B; }   // Peq of one job: word (k, c) of lane l at (4 k + c) * 64 + l

// one block, one column: Eq the block's match bits of the column's symbol, hin / hout in {-1, 0, +1}, top the bit of the block's last row
MM_HD int bv_block(uint32_t Eq, uint32_t& Pv, uint32_t& Mv, int hin, uint32_t top) {
  const uint32_t neg = hin < 0 ? 1u : 0u, pos = hin > 0 ? 1u : 0u;
  const uint32_t Xv = Eq | Mv;
  Eq |= neg;
  const uint32_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
  uint32_t Ph = Mv | ~(Xh | Pv), Mh = Pv & Xh;
  const int hout = (Ph & top) ? 1 : (Mh & top) ? -1 : 0;          // (garbage above top never flows down: carries and shifts go up)
  Ph = (Ph << 1) | pos; Mh = (Mh << 1) | neg;
  Pv = Mh | ~(Xv | Ph); Mv = Ph & Xv;
  return hout;
}

// ---- strings --------------------------------------------------------------------------------------------------------------------------------
// A source gives sym(p): edit_sym of stored base p.  BvBytes: ASCII on the host.
struct BvBytes {
  const char* s;
  MM_HD uint32_t sym(int64_t p) const { return edit_sym((uint8_t)s[p]); }
};
// the oriented string of a pass: stored bases [org, org + len), forward or (rc) reverse-complemented, then (rev) read from its end
template <class Src> struct BvString {
  Src src; int64_t org; int32_t len; bool rc, rev;
  MM_HD uint32_t at(int32_t i) const {
    if (rev) i = len - 1 - i;
    if (!rc) return src.sym(org + i);
    const uint32_t y = src.sym(org + len - 1 - i);
    return y > 3 ? (uint32_t)BV_SYM_NONE : 3u - y;
  }
};

// ---- one pass -------------------------------------------------------------------------------------------------------------------------------
struct BvPass { int32_t m, n, blocks, B, last_lane, hin0; uint32_t top; };
MM_HD BvPass bv_pass(int32_t m, int32_t n, bool anchored) {
  BvPass P;
  P.m = m; P.n = n; P.blocks = bv_blocks(m); P.B = bv_per_lane(m);
  P.last_lane = P.blocks ? (P.blocks - 1) / P.B : 0;
  P.hin0 = anchored ? 1 : 0;
  P.top = 1u << ((m - 1) & (BV_W - 1));
  return P;
}
MM_HD int32_t bv_lane_blocks(const BvPass& P, int lane) { const int32_t left = P.blocks - lane * P.B; return left < 0 ? 0 : left > P.B ? P.B : left; }
MM_HD int32_t bv_steps(const BvPass& P) { return P.n + BV_LANES - 1; }                 // steps 0 .. n + 62: lane 63 works on column n - 1 at the last one
MM_HD int32_t bv_column(int32_t t, int lane) { return t - lane; }                      // the fill: lane l starts at step l; the drain: it ends at step n - 1 + l
MM_HD uint32_t bv_msg(uint32_t sym, int h) { return sym | (uint32_t)(h + 1) << 3; }    // what a lane hands to the next: the column's symbol and hout
MM_HD uint32_t bv_msg_sym(uint32_t w) { return w & 7u; }
MM_HD int bv_msg_h(uint32_t w) { return (int)(w >> 3) - 1; }

template <int BT> struct BvLane { uint32_t pv[BT], mv[BT]; int32_t nb, score, best, col; };

// the lane's blocks of Peq (peq: the job's words, already offset by the lane), Pv, Mv and the score
template <int BT, class Q> MM_HD void bv_lane_init(const BvPass& P, int lane, const Q& q, uint32_t* peq, BvLane<BT>& L) {
  L.nb = bv_lane_blocks(P, lane); L.score = P.m; L.best = P.m; L.col = 0;
MM_BV_UNROLL
  for (int k = 0; k < BT; ++k) {
    L.pv[k] = ~0u; L.mv[k] = 0;
    if (k < L.nb) {
      uint32_t e0 = 0, e1 = 0, e2 = 0, e3 = 0;
      const int32_t i0 = (lane * P.B + k) * BV_W, rows = P.m - i0 < BV_W ? P.m - i0 : BV_W;
      for (int i = 0; i < rows; ++i) {
        const uint32_t y = q.at(i0 + i), bit = 1u << i;
        e0 |= y == 0 ? bit : 0u; e1 |= y == 1 ? bit : 0u; e2 |= y == 2 ? bit : 0u; e3 |= y == 3 ? bit : 0u;
      }
      uint32_t* w = peq + (size_t)(4 * k) * BV_LANES;
      w[0] = e0; w[BV_LANES] = e1; w[2 * BV_LANES] = e2; w[3 * BV_LANES] = e3;
    }
  }
}

// step t of one lane: in is the word of lane - 1's previous step (lane 0: the window's symbol with the pass's hin); returns the word for lane + 1
template <int BT> MM_HD uint32_t bv_lane_step(const BvPass& P, int lane, int32_t t, uint32_t in, const uint32_t* peq, BvLane<BT>& L) {
  const int32_t j = bv_column(t, lane);
  if (j < 0 || j >= P.n || L.nb == 0) return in;
  const uint32_t sym = bv_msg_sym(in), hit = sym < 4 ? ~0u : 0u;
  const uint32_t* w = peq + (size_t)(sym & 3u) * BV_LANES;
  int h = bv_msg_h(in);
MM_BV_UNROLL
  for (int k = 0; k < BT; ++k)
    if (k < L.nb) h = bv_block(w[(size_t)(4 * k) * BV_LANES] & hit, L.pv[k], L.mv[k], h, lane == P.last_lane && k == L.nb - 1 ? P.top : 1u << (BV_W - 1));
  if (lane == P.last_lane) {
    L.score += h;
    if (L.score < L.best) { L.best = L.score; L.col = j + 1; }
  }
  return bv_msg(sym, h);
}

// One pass on the lanes G: the smallest bottom-row score and the first column that has it, the same in every lane.  peq: bv_peq_words(P.B) words.
// G gives HELD (lanes per thread), lane(h), up(v, o) (o[h] = the v of the lane below lane(h); unspecified for lane 0) and pick(v, l) (lane l's v).
template <int BT, class G, class Q, class R> MM_HD void bv_run_pass(const G& g, const BvPass& P, const Q& q, const R& r, uint32_t* peq, int32_t* best, int32_t* col) {
  BvLane<BT> L[G::HELD];
  uint32_t out[G::HELD], in[G::HELD], text[G::HELD];
  for (int h = 0; h < G::HELD; ++h) { bv_lane_init<BT>(P, g.lane(h), q, peq + g.lane(h), L[h]); out[h] = 0; text[h] = BV_SYM_NONE; }
  const int32_t steps = P.blocks ? bv_steps(P) : 0;               // (m = 0: no block; the score stays 0 at column 0)
  for (int32_t t = 0; t < steps; ++t) {
    if ((t & (BV_LANES - 1)) == 0)                                // the window's next 64 columns, one per lane
      for (int h = 0; h < G::HELD; ++h) { const int32_t j = t + g.lane(h); text[h] = j < P.n ? r.at(j) : (uint32_t)BV_SYM_NONE; }
    g.up(out, in);
    const uint32_t s0 = g.pick(text, t & (BV_LANES - 1));
    for (int h = 0; h < G::HELD; ++h) if (g.lane(h) == 0) in[h] = bv_msg(s0, P.hin0);
    for (int h = 0; h < G::HELD; ++h) out[h] = bv_lane_step<BT>(P, g.lane(h), t, in[h], peq + g.lane(h), L[h]);
  }
  int32_t b[G::HELD], c[G::HELD];
  for (int h = 0; h < G::HELD; ++h) { b[h] = L[h].best; c[h] = L[h].col; }
  *best = (int32_t)g.pick(b, P.last_lane); *col = (int32_t)g.pick(c, P.last_lane);
}

// d, a, b of a job: the stored read [q_org, q_org + m) of qs on `strand` against the window [r_org, r_org + n) of rs; *dist = -1: not aligned
template <int BT, class G, class QS, class RS>
MM_HD void bv_align(const G& g, const QS& qs, int64_t q_org, int32_t m, int strand, const RS& rs, int64_t r_org, int32_t n, int32_t max_dist, uint32_t* peq,
                    int32_t* dist, int32_t* a, int32_t* b) {
  *dist = -1; *a = 0; *b = 0;
  if (m > EDIT_MAX_READ) return;
  int32_t d = 0, e = 0, d2 = 0, e2 = 0;
  bv_run_pass<BT>(g, bv_pass(m, n, false), BvString<QS>{qs, q_org, m, strand < 0, false}, BvString<RS>{rs, r_org, n, false, false}, peq, &d, &e);
  if (d > max_dist) return;
  bv_run_pass<BT>(g, bv_pass(m, e, true), BvString<QS>{qs, q_org, m, strand < 0, true}, BvString<RS>{rs, r_org, e, false, true}, peq, &d2, &e2);
  *dist = d; *b = e; *a = e - e2;                                 // (d2 == d: the best alignment that ends at b costs d)
}

// ---- the serial form: one column after the other, the blocks top to bottom (st: 6 * blocks words) ----
template <class Q, class R> MM_HD void bv_serial_pass(int32_t m, int32_t n, bool anchored, const Q& q, const R& r, uint32_t* st, int32_t* best, int32_t* col) {
  const int32_t nb = bv_blocks(m);
  uint32_t* peq = st; uint32_t* pv = st + 4 * (size_t)nb; uint32_t* mv = pv + nb;
  for (int32_t k = 0; k < 4 * nb; ++k) peq[k] = 0;
  for (int32_t i = 0; i < m; ++i) { const uint32_t y = q.at(i); if (y < 4) peq[4 * (i / BV_W) + y] |= 1u << (i % BV_W); }
  for (int32_t k = 0; k < nb; ++k) { pv[k] = ~0u; mv[k] = 0; }
  int32_t score = m; *best = m; *col = 0;
  for (int32_t j = 0; j < n && nb; ++j) {
    const uint32_t y = r.at(j);
    int h = anchored ? 1 : 0;
    for (int32_t k = 0; k < nb; ++k) h = bv_block(y < 4 ? peq[4 * k + y] : 0u, pv[k], mv[k], h, k == nb - 1 ? 1u << ((m - 1) & (BV_W - 1)) : 1u << (BV_W - 1));
    score += h;
    if (score < *best) { *best = score; *col = j + 1; }
  }
}

}  // namespace mm

// ---- the whole definition on one host thread, both forms (the tests' host build; tools/edit_host_align.cpp) ----
#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>

namespace mm {

struct BvHostLanes {                                              // the 64 lanes of a wavefront in plain loops
  static constexpr int HELD = BV_LANES;
  int lane(int h) const { return h; }
  template <class T> void up(const T* v, T* o) const { o[0] = 0; for (int h = 1; h < HELD; ++h) o[h] = v[h - 1]; }
  template <class T> T pick(const T* v, int l) const { return v[l]; }
};

// read: L bytes as stored (strand -1: aligned as its reverse complement); window: the n bytes of contig[ws, we)
inline EditHostResult bv_infix_host(const char* read, int64_t L, int strand, const char* window, int64_t n, int32_t max_dist, bool pipeline) {
  EditHostResult res{-1, 0, 0};
  if (L > EDIT_MAX_READ) return res;
  const int32_t m = (int32_t)L;
  int32_t d = -1, a = 0, b = 0;
  const BvBytes qs{read}, rs{window};
  if (pipeline) {
    std::vector<uint32_t> peq((size_t)bv_peq_words(bv_per_lane(m)) + 1);
    const BvHostLanes g;
    switch (bv_class(bv_per_lane(m))) {
      case 1: bv_align<1>(g, qs, 0, m, strand, rs, 0, (int32_t)n, max_dist, peq.data(), &d, &a, &b); break;
      case 2: bv_align<2>(g, qs, 0, m, strand, rs, 0, (int32_t)n, max_dist, peq.data(), &d, &a, &b); break;
      case 4: bv_align<4>(g, qs, 0, m, strand, rs, 0, (int32_t)n, max_dist, peq.data(), &d, &a, &b); break;
      case 8: bv_align<8>(g, qs, 0, m, strand, rs, 0, (int32_t)n, max_dist, peq.data(), &d, &a, &b); break;
      case 16: bv_align<16>(g, qs, 0, m, strand, rs, 0, (int32_t)n, max_dist, peq.data(), &d, &a, &b); break;
      default: bv_align<32>(g, qs, 0, m, strand, rs, 0, (int32_t)n, max_dist, peq.data(), &d, &a, &b); break;
    }
  } else {
    std::vector<uint32_t> st((size_t)6 * (size_t)bv_blocks(m) + 1);
    int32_t e = 0, d2 = 0, e2 = 0;
    bv_serial_pass(m, (int32_t)n, false, BvString<BvBytes>{qs, 0, m, strand < 0, false}, BvString<BvBytes>{rs, 0, (int32_t)n, false, false}, st.data(), &d, &e);
    if (d <= max_dist) {
      bv_serial_pass(m, e, true, BvString<BvBytes>{qs, 0, m, strand < 0, true}, BvString<BvBytes>{rs, 0, e, false, true}, st.data(), &d2, &e2);
      b = e; a = e - e2;
    } else d = -1;
  }
  res.dist = d; res.begin = a; res.end = b;
  return res;
}

}  // namespace mm
#endif
