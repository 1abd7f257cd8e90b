// Base modifications (the MM/ML tags of a read; SAM tags specification, "Base modifications") per reference position ("Base
// modifications"), written once for the kernels of mm_mods.hip (one wavefront per read, per job) and for the host (plain g++: tests/test_mods_core.cpp
// holds it to tests/mods_ref.py).
//
//   groups   a read has groups in MM order, one code each: base (A 0, C 1, G 2, T 3), code (the index 0..3 of its code among the asked ones, -1 for any
//            other), mode ('.', '?' or 0 for absent), and n skips with n ML bytes.  Skips s0, s1, .. name the occurrences o_j = sum_{i <= j} (s_i + 1),
//            1-based, among the read's bases whose upper-cased byte is the group's base.  The sums are 64-bit and stored saturated to 32 bits: an
//            ordinal beyond the read's count of the base is an error whatever its value.
//   plane    two bytes per base, who | prob << 8, in the order the set holds the read.  At a base of letter B every group of base B gives its ML byte
//            if the base is one of its occurrences, else 0 if its mode is '.' or absent, else nothing.  Nothing at all: 0.  Else S = min(255, sum p),
//            pc = 255 - S, g* the first group with the largest p: pc >= p(g*) gives who 1 (canonical) and prob pc, else who 3 + code (2 for code -1)
//            and prob p(g*).
//   events   walking a job's runs as mm_pileup_core.hpp does (r = first, i = 0): column t of an = run reads the stored base s = i + t (strand +) or
//            m - 1 - (i + t) (strand -); who[s] != 0 gives one event (contig, r + t, strand, class), class 1 (fail) if prob[s] < T, else 0 for
//            canonical, 2 for other, 3 + code.  X, I and D runs give none.  A job's events are emitted in no particular order: they are sorted.
//   key      contig << 36 | pos << 4 | (strand < 0) << 3 | class.  2^28 contigs at most.
//   rows     the at most 7 entries of a (contig, pos, strand) segment of a merged table, with b the reference's byte there, upper-cased, complemented
//            for strand -: b outside ACGT gives nothing; every asked code k whose base is b, in their order, gives N_mod = count of class 3 + k,
//            N_canonical = class 0, N_other = class 2 plus the other asked codes, N_fail = class 1; kept iff N_mod + N_canonical + N_other >= the
//            minimal coverage.
//
// The lane policy P is mm_pileup_core.hpp's (P::W, lane, scan_add, ballot, pick).  Bounds: group_ordinals reads skips[0, n) and writes ord[0, n);
// plane_read reads q.byte(0 .. L - 1) and, of the groups [g0, g1), ord and ml at [soff[g], soff[g + 1]) only, and writes out[0, L) — an ordinal is
// compared, never used as an index; walk_job reads ops[0, n_ops) and m.call(0 .. mlen - 1) after mmp::count_job's checks have passed and writes
// out[0, events), events the value it returned with out == nullptr.
#pragma once
#include "mm_pileup_core.hpp"

namespace mmd {

constexpr uint32_t WHO_NONE = 0, WHO_CANONICAL = 1, WHO_OTHER = 2, WHO_CODE0 = 3;
constexpr uint32_t CLASS_CANONICAL = 0, CLASS_FAIL = 1, CLASS_OTHER = 2, CLASS_CODE0 = 3, N_CLASSES = 7;
constexpr int MAX_CODES = 4, MAX_GROUPS = 255;                    // asked codes; groups of one read (the error word holds the group in 8 bits)
constexpr uint8_t MODE_ABSENT = 0, MODE_DOT = '.', MODE_ASK = '?';
constexpr int POS_SHIFT = 4, CONTIG_SHIFT = 36;
constexpr int64_t MAX_CONTIGS = (int64_t)1 << 28;
constexpr uint32_t ORD_SAT = 0xFFFFFFFFu;
constexpr int32_t DEFAULT_MIN_ML = 204;                           // a declared default: ML bytes 204..255 are p >= 0.797

MM_HD uint64_t make_key(int64_t contig, int64_t pos, int32_t strand, uint32_t cls) {
  return (uint64_t)contig << CONTIG_SHIFT | (uint64_t)pos << POS_SHIFT | (uint64_t)(strand < 0 ? 8 : 0) | cls;
}
MM_HD int64_t key_contig(uint64_t key) { return (int64_t)(key >> CONTIG_SHIFT); }
MM_HD int64_t key_pos(uint64_t key) { return (int64_t)(key >> POS_SHIFT & 0xFFFFFFFFull); }
MM_HD bool key_minus(uint64_t key) { return (key >> 3 & 1) != 0; }
MM_HD uint32_t key_class(uint64_t key) { return (uint32_t)(key & 7u); }
MM_HD uint64_t key_site(uint64_t key) { return key >> 3; }        // contig, position and strand
MM_HD uint32_t below(uint64_t mask, uint32_t lane) { return (uint32_t)__builtin_popcountll(mask & (((uint64_t)1 << lane) - 1)); }
MM_HD uint32_t popc(uint64_t mask) { return (uint32_t)__builtin_popcountll(mask); }

// the groups of a set, one behind the other: group g has the skips, ordinals and ML bytes [soff[g], soff[g + 1])
struct Groups { const uint8_t* base; const int8_t* code; const uint8_t* mode; const int64_t* soff; const uint32_t* ord; const uint8_t* ml; };

// the ordinals of one group's n skips, saturated
template <class P> MM_HD void group_ordinals(P& p, const uint32_t* skips, int64_t n, uint32_t* ord) {
  int64_t run = 0;                                                 // (n < 2^31 skips of less than 2^32 each: no wrap in 64 bits)
  for (int64_t k0 = 0; k0 < n; k0 += P::W) {
    const int64_t k = k0 + p.lane();
    const int64_t v = k < n ? (int64_t)skips[k] + 1 : 0;
    int64_t tot;
    const int64_t o = run + p.scan_add(v, &tot) + v;
    run += tot;
    if (k < n) ord[k] = o > (int64_t)ORD_SAT ? ORD_SAT : (uint32_t)o;
  }
}

MM_HD uint16_t call_of(uint32_t sum, uint32_t best, int code) {
  const uint32_t pc = 255u - (sum > 255u ? 255u : sum);
  if (pc >= best) return (uint16_t)(WHO_CANONICAL | pc << 8);
  return (uint16_t)((code >= 0 ? WHO_CODE0 + (uint32_t)code : WHO_OTHER) | best << 8);
}

// the plane of a read of L bases with the groups [g0, g1), whose ordinals are written; returns the lowest group (counted from g0) that names an
// occurrence beyond the read's count of its base, or -1 (the same in every lane)
template <class P, class Q> MM_HD int plane_read(P& p, const Q& q, int64_t L, const Groups& G, int64_t g0, int64_t g1, uint16_t* out) {
  int64_t seen[4] = {0, 0, 0, 0};                                  // the letters before this tile: the same in every lane
  for (int64_t j0 = 0; j0 < L; j0 += P::W) {
    const int64_t j = j0 + p.lane();
    const uint32_t c = j < L ? mmp::base_code(q.byte(j)) : mmp::CODE_N;
    uint32_t mine = 0;                                             // this base's ordinal among its letter
    for (uint32_t x = 0; x < 4; ++x) {
      const uint64_t mask = p.ballot(c == x);
      if (c == x) mine = (uint32_t)seen[x] + below(mask, p.lane()) + 1;
      seen[x] += popc(mask);
    }
    if (j >= L) continue;
    uint32_t sum = 0, best = 0;
    int64_t star = -1;
    if (c < 4)
      for (int64_t g = g0; g < g1; ++g) {
        if (G.base[g] != c) continue;
        const int64_t lo = G.soff[g], n = G.soff[g + 1] - lo;
        int64_t a = 0, b = n;                                      // the first ordinal >= mine
        while (a < b) { const int64_t mid = a + (b - a) / 2; if (G.ord[lo + mid] < mine) a = mid + 1; else b = mid; }
        uint32_t pr = 0;
        if (a < n && G.ord[lo + a] == mine) pr = G.ml[lo + a];
        else if (G.mode[g] == MODE_ASK) continue;
        sum += pr;
        if (star < 0 || pr > best) { best = pr; star = g; }
      }
    out[j] = star < 0 ? (uint16_t)0 : call_of(sum, best, G.code[star]);
  }
  int bad = -1;
  for (int64_t g = g1; g-- > g0;) {
    const int64_t lo = G.soff[g], n = G.soff[g + 1] - lo;
    if (n > 0 && (int64_t)G.ord[lo + n - 1] > seen[G.base[g]]) bad = (int)(g - g0);
  }
  return bad;
}

// the class of a stored call v != 0 under the threshold T (0..255)
MM_HD uint32_t class_of(uint16_t v, int32_t T) {
  const uint32_t who = v & 255u;
  return (int32_t)(v >> 8) < T ? CLASS_FAIL : who == WHO_CANONICAL ? CLASS_CANONICAL : who;
}
template <class M> MM_HD uint16_t oriented_call(const M& m, int64_t mlen, int32_t strand, int64_t i) { return m.call(strand < 0 ? mlen - 1 - i : i); }

// The events of a job whose checks have passed, to out[0, events) — out == nullptr: counted only; returns their number (the same in every lane).
// A lane takes an = run of up to LONG_RUN columns, all lanes a longer one.
template <class P, class M> MM_HD int64_t walk_job(P& p, const M& m, int64_t mlen, int32_t strand, int64_t contig, int64_t first, const uint32_t* ops, int64_t n_ops, int32_t T,
                                                  uint64_t* out) {
  int64_t rsum = 0, isum = 0, at = 0;                              // the running values: the same in every lane
  for (int64_t base = 0; base < n_ops; base += P::W) {
    const mmp::Run x = mmp::run_of(ops, base + p.lane(), n_ops);
    int64_t tot;
    const int64_t r = first + rsum + p.scan_add(x.good && x.op != mmb::OP_I ? x.len : 0, &tot); rsum += tot;
    const int64_t i = isum + p.scan_add(x.good && x.op != mmb::OP_D ? x.len : 0, &tot); isum += tot;
    const bool eq = x.good && x.op == mmb::OP_EQ, wide = eq && x.len > mmp::LONG_RUN;
    int64_t mine = 0;
    if (eq && !wide) for (int64_t t = 0; t < x.len; ++t) mine += (oriented_call(m, mlen, strand, i + t) & 255u) != 0;
    int64_t o = at + p.scan_add(mine, &tot); at += tot;
    if (out && mine)
      for (int64_t t = 0; t < x.len; ++t) {
        const uint16_t v = oriented_call(m, mlen, strand, i + t);
        if (v & 255u) out[o++] = make_key(contig, r + t, strand, class_of(v, T));
      }
    for (uint64_t left = p.ballot(wide); left; left &= left - 1) {   // the long runs of the tile, one after the other, by all lanes
      uint32_t l = 0;
      while (!(left >> l & 1)) ++l;
      const int64_t lr = p.pick(r, l), li = p.pick(i, l), ln = p.pick(x.len, l);
      for (int64_t t0 = 0; t0 < ln; t0 += P::W) {
        const int64_t t = t0 + p.lane();
        const uint16_t v = t < ln ? oriented_call(m, mlen, strand, li + t) : (uint16_t)0;
        const uint64_t mask = p.ballot((v & 255u) != 0);
        if (out && (v & 255u)) out[at + below(mask, p.lane())] = make_key(contig, lr + t, strand, class_of(v, T));
        at += popc(mask);
      }
    }
  }
  return at;
}

MM_HD uint8_t complement_letter(uint8_t b) { return b == 'A' ? 'T' : b == 'C' ? 'G' : b == 'G' ? 'C' : b == 'T' ? 'A' : 0; }

struct CodeBases { uint8_t b[MAX_CODES]; int n; };                // the base letter of every asked code
struct Row { uint64_t site, n_mod, n_canonical, n_other, n_fail; };   // site: contig << 36 | pos << 4 | (strand < 0) << 3 | the code's index
// the rows of the segment that entry i of the ascending unique keys[0, n) starts; ref_byte: the reference's byte at its position; out may be null
MM_HD int segment_rows(const uint64_t* keys, const uint32_t* counts, int64_t i, int64_t n, uint8_t ref_byte, const CodeBases& cb, int64_t min_coverage, Row* out) {
  uint64_t cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t e = i; e < n && e < i + (int64_t)N_CLASSES && key_site(keys[e]) == key_site(keys[i]); ++e) cnt[key_class(keys[e])] = counts[e];
  uint8_t b = mmb::upper(ref_byte);
  b = key_minus(keys[i]) ? complement_letter(b) : complement_letter(complement_letter(b));   // (0 for a byte outside ACGT)
  if (!b) return 0;
  int rows = 0;
  for (int k = 0; k < cb.n; ++k) {
    if (cb.b[k] != b) continue;
    uint64_t other = cnt[CLASS_OTHER];
    for (int o = 0; o < cb.n; ++o) if (o != k) other += cnt[CLASS_CODE0 + (uint32_t)o];
    const uint64_t mod = cnt[CLASS_CODE0 + (uint32_t)k], canon = cnt[CLASS_CANONICAL];
    if (mod + canon + other < (uint64_t)min_coverage) continue;
    if (out) out[rows] = Row{(keys[i] & ~(uint64_t)7) | (uint64_t)k, mod, canon, other, cnt[CLASS_FAIL]};
    ++rows;
  }
  return rows;
}

}  // namespace mmd
