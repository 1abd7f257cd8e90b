// Which annotated genes does a mapping overlap (classify --genes; DESIGN.md section 4, "Gene-level analysis"): the stabbing query over the genes
// of one contig, and the checks on the arguments of mm_gene_overlap.
//   genes     of all contigs, sorted by (contig, Start): genes of contig c are [off[c], off[c+1]); start[], stop[] (both inclusive, as in
//             DB_annotations.txt); pmax[j] = the largest stop among the contig's genes up to j (gene_prefix_max, built on the host)
//   overlap   gene (Start, Stop) and mapping (s, e) of one contig overlap iff Start < e && s <= Stop
// For a mapping (c, s, e) the candidates are one range of genes: hi = the first gene of c with Start >= e, lo = the first gene of c with
// pmax >= s (pmax ascends within a contig: below lo no gene reaches s, from hi on none starts before e) — two binary searches (gene_span).
// Gene j of [lo, hi) is reported iff stop[j] >= s.  gene_stab walks the range from hi - 1 downwards; lane l of `width` lanes takes hi - 1 - l,
// hi - 1 - l - width, ...; the visitor is called by every lane in every step, with hit or not, so that lanes that share a mapping can place
// what they report (G::place) — one text for a serial caller, a lane that owns a mapping, and a wavefront striding over one.  Counting and
// emitting are two visitors of the same walk and cannot disagree.
//
// Compiles for host (tests/test_gene_core.cpp via g++, tools/gene_host_join.cpp) and device (mm_gene.hip).
#pragma once
#include <stdint.h>

#ifndef MM_HD
#if defined(__HIPCC__)
#define MM_HD __host__ __device__ inline
#else
#define MM_HD inline
#endif
#endif

namespace mm {

struct GeneTable { const int64_t* off; const int32_t* start; const int32_t* stop; const int32_t* pmax; };

MM_HD bool gene_overlaps(int32_t g_start, int32_t g_stop, int32_t s, int32_t e) { return g_start < e && s <= g_stop; }

// pmax of the genes of every contig (pmax may alias nothing of the inputs)
inline void gene_prefix_max(int64_t n_contigs, const int64_t* off, const int32_t* stop, int32_t* pmax) {
  for (int64_t c = 0; c < n_contigs; ++c) {
    int32_t m = INT32_MIN;
    for (int64_t j = off[c]; j < off[c + 1]; ++j) { m = stop[j] > m ? stop[j] : m; pmax[j] = m; }
  }
}

// first index of the ascending a[lo, hi) with a[j] >= x (hi if none)
MM_HD int64_t gene_lower_bound(const int32_t* a, int64_t lo, int64_t hi, int32_t x) {
  while (lo < hi) { const int64_t mid = lo + (hi - lo) / 2; if (a[mid] < x) lo = mid + 1; else hi = mid; }
  return lo;
}
// the candidates [*lo, *hi) of mapping (c, s, e); empty ranges have *lo == *hi
MM_HD void gene_span(const GeneTable& T, int32_t c, int32_t s, int32_t e, int64_t* lo, int64_t* hi) {
  const int64_t a = T.off[c], b = T.off[c + 1];
  *hi = gene_lower_bound(T.start, a, b, e);
  *lo = gene_lower_bound(T.pmax, a, *hi, s);
}

// one lane on its own: reports are placed one behind the other
struct GeneSerial {
  MM_HD int lane() const { return 0; }
  MM_HD int width() const { return 1; }
  MM_HD int place(bool hit, int* total) const { *total = hit ? 1 : 0; return 0; }   // my report's place among this step's, and how many there are
};

// v(g, j, hit) for every lane in every step; the reports of one mapping come in descending j whatever the width
template <class G, class V> MM_HD void gene_stab(const G& g, const GeneTable& T, int64_t lo, int64_t hi, int32_t s, V& v) {
  for (int64_t top = hi - 1; top >= lo; top -= g.width()) {
    const int64_t j = top - g.lane();
    v(g, j, j >= lo && T.stop[j] >= s);
  }
}

struct GeneCount {                                                // overlaps, and the feature ids behind them (foff: per group, may be null)
  const int32_t* group; const int64_t* foff; int64_t n = 0, nk = 0;
  template <class G> MM_HD void operator()(const G&, int64_t j, bool hit) {
    if (!hit) return;
    ++n;
    if (foff) nk += foff[group[j] + 1] - foff[group[j]];
  }
};
struct GeneEmit {                                                 // the overlapped genes, from out[at] on
  int64_t* out; int64_t at = 0;
  template <class G> MM_HD void operator()(const G& g, int64_t j, bool hit) {
    int total; const int k = g.place(hit, &total);
    if (hit) out[at + k] = j;
    at += total;
  }
};

// ---- the arguments of mm_gene_overlap (host): 0 if fine, else which rule is broken (gene_arg_message)
enum GeneArgError { GENE_OK = 0, GENE_BAD_OFFSETS, GENE_UNSORTED, GENE_STOP_BEFORE_START, GENE_BAD_GROUP, GENE_BAD_FEAT_OFFSETS, GENE_BAD_FEATURE,
                    GENE_BAD_MAP_CONTIG, GENE_MAP_STOP_BEFORE_START, GENE_BAD_IDENTITY };
inline const char* gene_arg_message(int e) {
  static const char* const M[] = {"", "gene table: contig_gene_off must start at 0 and ascend", "gene table: genes are not sorted by Start within a contig",
                                  "gene table: a gene's Stop lies before its Start", "gene table: a gene_group lies outside [0, n_groups)",
                                  "gene table: group_feat_off must start at 0 and ascend", "gene table: a feature id lies outside [0, n_feats)",
                                  "mappings: a map_contig lies outside [0, n_contigs)", "mappings: a map_stop lies before its map_start",
                                  "mappings: an identity is negative or not a number"};
  return e >= 0 && e < (int)(sizeof M / sizeof M[0]) ? M[e] : "?";
}
inline int gene_table_check(int64_t n_contigs, const int64_t* off, const int32_t* start, const int32_t* stop, const int32_t* group, int64_t n_groups,
                            const int64_t* foff, const int32_t* feat, int64_t n_feats) {
  if (n_contigs < 0 || n_groups < 0 || n_feats < 0 || !off || off[0] != 0) return GENE_BAD_OFFSETS;
  for (int64_t c = 0; c < n_contigs; ++c) if (off[c + 1] < off[c]) return GENE_BAD_OFFSETS;
  for (int64_t c = 0; c < n_contigs; ++c)
    for (int64_t j = off[c]; j < off[c + 1]; ++j) {
      if (j > off[c] && start[j] < start[j - 1]) return GENE_UNSORTED;
      if (stop[j] < start[j]) return GENE_STOP_BEFORE_START;
      if (group[j] < 0 || group[j] >= n_groups) return GENE_BAD_GROUP;
    }
  if (!foff || foff[0] != 0) return GENE_BAD_FEAT_OFFSETS;
  for (int64_t g = 0; g < n_groups; ++g) if (foff[g + 1] < foff[g]) return GENE_BAD_FEAT_OFFSETS;
  for (int64_t k = 0; k < foff[n_groups]; ++k) if (feat[k] < 0 || feat[k] >= n_feats) return GENE_BAD_FEATURE;
  return GENE_OK;
}
inline int gene_maps_check(int64_t n_maps, const int32_t* contig, const int32_t* s, const int32_t* e, const double* ident, int64_t n_contigs) {
  for (int64_t m = 0; m < n_maps; ++m) {
    if (contig[m] < 0 || contig[m] >= n_contigs) return GENE_BAD_MAP_CONTIG;
    if (e[m] < s[m]) return GENE_MAP_STOP_BEFORE_START;
    if (!(ident[m] >= 0)) return GENE_BAD_IDENTITY;                // (a NaN is refused)
  }
  return GENE_OK;
}

}  // namespace mm
