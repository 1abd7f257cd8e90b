// Exact edit distances of mappings (not in the reference; DESIGN.md section 1, "Edit distances"): the definition, and the one text of the alignment for
// the host build and for a device build (the device path runs mm_edit_bv_core.hpp against this definition; this routine stays host-only: DESIGN.md says why).
//   record       read r of length L on contig c of length C at ref_start, strand +1 / -1
//   Q            the read; for strand -1 its reverse complement.  m = L
//   window       R = contig[ws, we), ws = max(0, ref_start - pad), we = min(C, ref_start + L + pad), pad = 64 + L / 16.  n = we - ws
//   bases        bytes compare upper-cased; A C G T match the same letter, every other byte matches nothing (not even itself, nor as a complement)
//   cap          floor(1.5 * L * (100 - pi) / 100) in double, pi the run's --pi
//   d            min over 0 <= a <= b <= n of the unit-cost Levenshtein distance of Q and R[a, b) (the read global, the window's ends free)
//   b            the smallest end at which some R[a, b) has distance d;  a: the largest start with Lev(Q, R[a, b)) = d
//   not aligned  d > cap, or L > EDIT_MAX_READ
// The alignment of a job that is aligned (mapDirectly --paf; mm_edit_trace_core.hpp computes it; DESIGN.md section 1, "Alignments"):
//   T, E         T = window[a, b) of length n = b - a.  E[i][j] = the unit-cost edit distance of Q[i, m) to T[j, n): E[m][j] = n - j, E[i][n] = m - i,
//                E[0][0] = d.  Bases match as above
//   walk         from (0, 0) to (m, n), at each cell the first of these that applies:
//                  =  if i < m, j < n and Q[i] matches T[j]                  -> (i + 1, j + 1)
//                  X  if i < m, j < n and E[i + 1][j + 1] + 1 == E[i][j]     -> (i + 1, j + 1)
//                  I  if i < m and E[i + 1][j] + 1 == E[i][j]                -> (i + 1, j)       it consumes a read base
//                  D  otherwise                                             -> (i, j + 1)       it consumes a window base
//   runs         equal neighbouring operations merged, each one word as BAM has them: len << 4 | op, I = 1, D = 2, = = 7, X = 8
//   follows      the X + I + D bases are d; = + X + I = m and = + X + D = n; at most 2 d + 1 runs (d edits separate at most d + 1 runs of =); the first
//                and the last run are never D (b is the smallest end and a the largest start at distance d)
//   no runs      a job that is not aligned, and m = 0
// Wavefront alignment (Marco-Sola et al. 2021) in its edit-distance form, without traceback.  Diagonal k = j - i; H_s[k] = the furthest read index i
// on diagonal k that s edits reach.  Pass 1 starts on every diagonal k >= 0 (the window's start is free), H_0[k] = extend(0, k), and goes
//   H_s[k] = extend(max(H_{s-1}[k] + 1, H_{s-1}[k-1], H_{s-1}[k+1] + 1)) clipped to i <= m and i + k <= n
// (clipping is exact: distances do not fall along a diagonal) until some H_s[k] = m: d = s, b = m + the smallest such k; s never passes the cap.
// Pass 2 is the same routine on the reversed strings reverse(Q), reverse(R[0, b)) from the one start diagonal 0 with the cap d: it reaches m at
// score d, and a = b - (m + the smallest k).  At score s only the diagonals [-s, n - m + cap - s] can still end inside the window; the others are
// not computed.  The two wavefront arrays hold edit_wave_words() words each: diagonals -cap - 1 .. n - m + cap + 1.
// Strings are packed: 16 bases per 32-bit word (base t at bits [2t, 2t + 2)) and one "matches nothing" bit per base, 32 per word, both forward;
// extend compares 16 bases per step (a funnel shift of two words, XOR, OR of the masks, count of trailing zeros; leading zeros in pass 2, which
// reads the forward words backwards).  The lanes G give lane(), width(), sync() (the other lanes' stores are visible) and first() (a ballot).
//
// Compiles for host (tests/test_edit_core.cpp via g++) and, under hipcc, for the device.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef MM_HD
#if defined(__HIPCC__)
#define MM_HD __host__ __device__ inline
#else
#define MM_HD inline
#endif
#endif

namespace mm {

constexpr int32_t EDIT_MAX_READ = 65536;                          // a longer read is not aligned (one job would have to be split over several waves)
constexpr int32_t EDIT_NEG = -(1 << 30);                          // a diagonal that no alignment has reached

MM_HD int64_t edit_pad(int64_t L) { return 64 + L / 16; }
MM_HD void edit_window(int64_t ref_start, int64_t L, int64_t C, int64_t* ws, int64_t* we) {
  const int64_t pad = edit_pad(L);
  int64_t a = ref_start - pad, b = ref_start + L + pad;
  a = a < 0 ? 0 : a > C ? C : a;
  b = b > C ? C : b < a ? a : b;
  *ws = a; *we = b;
}
MM_HD int32_t edit_cap(int64_t L, float pi) {
  const double c = floor(1.5 * (double)L * (100.0 - (double)pi) / 100.0);
  return c < 0 ? 0 : c > 2147483647.0 ? 2147483647 : (int32_t)c;
}
MM_HD int32_t edit_effective_cap(int32_t max_dist, int32_t m) { return max_dist < m ? max_dist : m; }   // (d <= m: an empty substring costs m)
MM_HD int64_t edit_wave_words(int64_t m, int64_t n, int32_t max_dist) {
  const int64_t cap = edit_effective_cap(max_dist, (int32_t)m), w = n - m + 2 * cap + 3;
  return w < 0 ? 0 : w;
}

// ---- bases -----------------------------------------------------------------------------------------------------------------------------------
MM_HD uint32_t edit_sym(uint8_t c) {                              // 0 .. 3: A C G T in either case; 4: matches nothing
  c &= 0xDF;
  return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
}
MM_HD uint32_t edit_spread16(uint32_t x) {                        // bit t -> bit 2t
  x = (x | (x << 8)) & 0x00FF00FFu; x = (x | (x << 4)) & 0x0F0F0F0Fu; x = (x | (x << 2)) & 0x33333333u; return (x | (x << 1)) & 0x55555555u;
}
MM_HD uint32_t edit_reverse_pairs(uint32_t x) {                   // base t -> base 15 - t
  x = (x >> 16) | (x << 16); x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
  x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4); return ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
}
MM_HD uint32_t edit_reverse16(uint32_t x) {                       // bit t -> bit 15 - t
  x = ((x >> 8) & 0x00FFu) | ((x & 0x00FFu) << 8); x = ((x >> 4) & 0x0F0Fu) | ((x & 0x0F0Fu) << 4);
  x = ((x >> 2) & 0x3333u) | ((x & 0x3333u) << 2); return ((x >> 1) & 0x5555u) | ((x & 0x5555u) << 1);
}

// A source gives codes16(p, &mask): the bases [p, p + 16) of a stored sequence, forward, as 2-bit codes and "matches nothing" bits (what lies
// behind the sequence's end is unspecified).  EditBytes: ASCII on the host.
struct EditBytes {
  const char* s; int64_t len;
  MM_HD uint32_t codes16(int64_t p, uint32_t* mask) const {
    uint32_t w = 0, k = 0;
    for (int t = 0; t < 16 && p + t < len; ++t) { const uint32_t y = edit_sym((uint8_t)s[p + t]); if (y > 3) k |= 1u << t; else w |= y << (2 * t); }
    *mask = k; return w;
  }
};
// the bases [p0, p0 + 16) of the oriented string: the sequence's [org, org + len) forward, or (rc; org = 0) its reverse complement; zero behind len
template <class Src> MM_HD uint32_t edit_pack16(const Src& src, int64_t org, int64_t len, bool rc, int64_t p0, uint32_t* mask) {
  const int64_t left = len - p0;
  if (left <= 0) { *mask = 0; return 0; }
  uint32_t w, k;
  if (!rc) w = src.codes16(org + p0, &k);
  else {
    const int64_t s0 = len - 16 - p0;                             // the 16 stored bases that end where the oriented ones begin
    const int sh = s0 < 0 ? (int)-s0 : 0;
    w = src.codes16(s0 < 0 ? 0 : s0, &k);
    w = ~edit_reverse_pairs(w << (2 * sh)); k = edit_reverse16((k << sh) & 0xFFFFu);
  }
  if (left < 16) { w &= (1u << (2 * left)) - 1u; k &= (1u << left) - 1u; }
  *mask = k & 0xFFFFu;
  return w;
}
// 32 bases from p0 (a multiple of 32): two code words and one mask word
template <class Src> MM_HD void edit_pack32(const Src& src, int64_t org, int64_t len, bool rc, int64_t p0, uint32_t* w2, uint32_t* mask) {
  uint32_t k0, k1;
  w2[0] = edit_pack16(src, org, len, rc, p0, &k0); w2[1] = edit_pack16(src, org, len, rc, p0 + 16, &k1);
  *mask = k0 | (k1 << 16);
}
MM_HD int64_t edit_groups(int64_t len) { return (len + 31) / 32 + 1; }   // groups of 32 bases that a packed string holds: one more than it needs, so that a fetch may read a word ahead
MM_HD int64_t edit_packed_words(int64_t len) { return 3 * edit_groups(len); }   // code words [0, 2g), mask words [2g, 3g)

// ---- the packed strings of one alignment -----------------------------------------------------------------------------------------------------
struct EditStrings { const uint32_t* qw; const uint32_t* qk; int32_t m; const uint32_t* rw; const uint32_t* rk; int32_t n; };

MM_HD uint32_t edit_shr(uint32_t lo, uint32_t hi, int sh) {       // the low word of hi:lo >> sh, 0 <= sh < 32
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(hi, lo, (uint32_t)sh);
#else
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
#endif
}
MM_HD uint32_t edit_codes_from(const uint32_t* w, int32_t p) { return edit_shr(w[p >> 4], w[(p >> 4) + 1], 2 * (p & 15)); }    // bases [p, p + 16)
MM_HD uint32_t edit_mask_from(const uint32_t* k, int32_t p) { return edit_shr(k[p >> 5], k[(p >> 5) + 1], p & 31) & 0xFFFFu; }
MM_HD uint32_t edit_codes_upto(const uint32_t* w, int32_t p) { return p >= 15 ? edit_codes_from(w, p - 15) : edit_codes_from(w, 0) << (2 * (15 - p)); }   // bases [p - 15, p], p in the top pair
MM_HD uint32_t edit_mask_upto(const uint32_t* k, int32_t p) { return p >= 15 ? edit_mask_from(k, p - 15) : (edit_mask_from(k, 0) << (15 - p)) & 0xFFFFu; }
MM_HD uint32_t edit_diff(uint32_t a, uint32_t b, uint32_t k) { const uint32_t x = a ^ b; return ((x | (x >> 1)) & 0x55555555u) | edit_spread16(k); }   // bit 2t: bases t differ

// how far read index i and window index j match on (at most limit bases); REV: of the reversed strings
template <bool REV> MM_HD int32_t edit_run(const EditStrings& S, int32_t i, int32_t j, int32_t limit) {
  int32_t run = 0;
  while (run < limit) {
    uint32_t x;
    if (!REV) {
      const int32_t p = i + run, q = j + run;
      x = edit_diff(edit_codes_from(S.qw, p), edit_codes_from(S.rw, q), edit_mask_from(S.qk, p) | edit_mask_from(S.rk, q));
    } else {
      const int32_t p = S.m - 1 - i - run, q = S.n - 1 - j - run;
      x = edit_diff(edit_codes_upto(S.qw, p), edit_codes_upto(S.rw, q), edit_mask_upto(S.qk, p) | edit_mask_upto(S.rk, q));
    }
    if (x) { run += (REV ? __builtin_clz(x) : __builtin_ctz(x)) >> 1; break; }
    run += 16;
  }
  return run < limit ? run : limit;
}

struct EditSerial {                                               // one lane on its own
  MM_HD int lane() const { return 0; }
  MM_HD int width() const { return 1; }
  MM_HD void sync() const {}
  MM_HD int first(bool hit) const { return hit ? 0 : -1; }        // the lowest lane with a hit, -1 if there is none
};

// The score at which the read's end is first reached (-1: not within cap) and *k_hit, the smallest diagonal that reaches it.  !REV: every start
// diagonal k >= 0 (pass 1); REV: the reversed strings from diagonal 0 (pass 2).  A, B: edit_wave_words(m, n, cap) words each.  Every lane of g
// makes the same calls and gets the same results.
template <bool REV, class G> MM_HD int32_t edit_wavefront(const G& g, const EditStrings& S, int32_t cap, int32_t* A, int32_t* B, int32_t* k_hit) {
  const int32_t m = S.m, n = S.n;
  cap = edit_effective_cap(cap, m);
  const int32_t kmax = n - m + cap, org = cap + 1, lane = g.lane(), width = g.width();
  if (cap < 0 || kmax < 0) return -1;                             // (d >= m - n)
  for (int32_t x = lane; x < kmax + cap + 3; x += width) { A[x] = EDIT_NEG; B[x] = EDIT_NEG; }
  g.sync();
  int32_t* prev = A; int32_t* cur = B;
  for (int32_t s = 0; s <= cap; ++s) {
    const int32_t lo = -s, hi = REV && s < kmax - s ? s : kmax - s;
    for (int32_t kb = lo; kb <= hi; kb += width) {
      const int32_t k = kb + lane;
      const bool on = k <= hi;
      int32_t v = EDIT_NEG;
      if (on) {
        if (s == 0) v = 0;
        else { const int32_t same = prev[org + k] + 1, below = prev[org + k - 1], above = prev[org + k + 1] + 1; v = same > below ? same : below; v = above > v ? above : v; }
        const int32_t room = n - k < m ? n - k : m;
        if (v > room) v = room;
        if (v < 0 || v + k < 0) v = EDIT_NEG;
        else { const int32_t qi = m - v, rj = n - k - v; v += edit_run<REV>(S, v, v + k, qi < rj ? qi : rj); }
        cur[org + k] = v;
      }
      const int f = g.first(on && v == m);
      if (f >= 0) { *k_hit = kb + f; return s; }
    }
    g.sync();
    int32_t* t = prev; prev = cur; cur = t;
  }
  return -1;
}

// d, a, b of the strings S (S.n: the whole window) within max_dist; *dist = -1: not aligned
template <class G> MM_HD void edit_align(const G& g, const EditStrings& S, int32_t max_dist, int32_t* A, int32_t* B, int32_t* dist, int32_t* a, int32_t* b) {
  int32_t k = 0, k2 = 0;
  *dist = -1; *a = 0; *b = 0;
  const int32_t d = edit_wavefront<false>(g, S, max_dist, A, B, &k);
  if (d < 0) return;
  EditStrings T = S;
  T.n = S.m + k;
  g.sync();
  if (edit_wavefront<true>(g, T, d, A, B, &k2) != d) return;      // (it is d: the best alignment that ends at b costs d)
  *dist = d; *b = T.n; *a = T.n - (S.m + k2);
}

// ---- the arguments of an alignment job (host): 0 if fine, else which rule is broken (edit_arg_message)
enum EditArgError { EDIT_OK = 0, EDIT_BAD_READ, EDIT_BAD_CONTIG, EDIT_BAD_STRAND, EDIT_BAD_MAX_DIST, EDIT_BAD_WINDOW };
inline const char* edit_arg_message(int e) {
  static const char* const M[] = {"", "a read lies outside the read set", "a contig lies outside the reference set", "a strand is neither +1 nor -1",
                                  "a negative max_dist", "a window ends before it starts or lies outside its contig"};
  return e >= 0 && e < (int)(sizeof M / sizeof M[0]) ? M[e] : "?";
}
inline int edit_job_check(int64_t read, int64_t strand, int64_t contig, int64_t max_dist, int64_t ws, int64_t we, int64_t n_reads, int64_t n_contigs, const int32_t* contig_len) {
  if (read < 0 || read >= n_reads) return EDIT_BAD_READ;
  if (contig < 0 || contig >= n_contigs) return EDIT_BAD_CONTIG;
  if (strand != 1 && strand != -1) return EDIT_BAD_STRAND;
  if (max_dist < 0) return EDIT_BAD_MAX_DIST;
  if (ws < 0 || we < ws || we > contig_len[contig]) return EDIT_BAD_WINDOW;
  return EDIT_OK;
}

}  // namespace mm

// ---- the whole definition on one host thread (the tests' host build) ----
#include <vector>

namespace mm {

struct EditHostResult { int32_t dist; int64_t begin, end; };       // window coordinates, half-open; dist -1: not aligned
// read: L bytes as stored (strand -1: aligned as its reverse complement); window: the n bytes of contig[ws, we)
inline EditHostResult edit_infix_host(const char* read, int64_t L, int strand, const char* window, int64_t n, int32_t max_dist) {
  EditHostResult r{-1, 0, 0};
  if (L > EDIT_MAX_READ) return r;
  const int64_t gq = edit_groups(L), gr = edit_groups(n);
  std::vector<uint32_t> q((size_t)(3 * gq)), w((size_t)(3 * gr));
  const EditBytes sq{read, L}, sr{window, n};
  for (int64_t g = 0; g < gq; ++g) edit_pack32(sq, 0, L, strand < 0, 32 * g, &q[(size_t)(2 * g)], &q[(size_t)(2 * gq + g)]);
  for (int64_t g = 0; g < gr; ++g) edit_pack32(sr, 0, n, false, 32 * g, &w[(size_t)(2 * g)], &w[(size_t)(2 * gr + g)]);
  const size_t words = (size_t)edit_wave_words(L, n, max_dist);
  std::vector<int32_t> A(words + 1), B(words + 1);
  const EditStrings S{q.data(), q.data() + 2 * gq, (int32_t)L, w.data(), w.data() + 2 * gr, (int32_t)n};
  int32_t a = 0, b = 0;
  edit_align(EditSerial{}, S, max_dist, A.data(), B.data(), &r.dist, &a, &b);
  r.begin = a; r.end = b;
  return r;
}

}  // namespace mm
