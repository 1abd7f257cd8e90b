// Confidence-thresholded lowest-common-ancestor assignment of a read (not in the reference; DESIGN.md section 4, "LCA assignment").
//   tree      nodes 0..n-1, parent[v] < v for v > 0, parent[0] == 0 (the root); tin / tout: Euler-tour numbers, a is in the subtree of v
//             iff tin[v] <= tin[a] < tout[v]
//   mass(v)   sum of the posteriors of the read's entries whose node lies in the subtree of v (v included), in double
//   lca       the deepest node with mass(v) >= tau - 1e-9; tau in [0.51, 1], so the qualifying nodes are one root-to-node chain; the root
//             if none qualifies
// How lca_read finds it, in passes over the read's entries that are sums, minima and maxima only (so one text serves a serial caller, a
// group of lanes with one entry each and a wavefront striding over a long read):
//   1. the total mass and the range of the entries' tin;
//   2. the weighted median of the entries in tin order, by bisection on the tin value: the smallest T with mass(tin <= T) >= total / 2.
//      A qualifying node holds more than half of the mass (0.51 - 1e-9 of a total that is 1 up to rounding; anything below 1.02 will do), so
//      its interval [tin, tout) contains T, with a margin of 0.01 of mass that no rounding of a sum reaches: the entry x with tin T lies
//      under the LCA;
//   3. from the node of x upwards until a node qualifies.  The root's mass is the total of step 1, summed in the same order.
// A sum that is exact in double does not depend on its order, so neither does the result for such posteriors.
//
// Compiles for host (unit tests: tests/test_lca_core.cpp via g++) and device (mm_lca.hip).
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

constexpr double LCA_SLACK = 1e-9;                                // absorbs posteriors that sum to 1 - ulp
MM_HD bool lca_threshold_ok(double tau) { return tau >= 0.51 && tau <= 1.0; }   // (a NaN is refused)
MM_HD bool lca_qualifies(double mass, double tau) { return mass >= tau - LCA_SLACK; }
MM_HD bool lca_in_subtree(int32_t tin_a, int32_t tin_v, int32_t tout_v) { return tin_a >= tin_v && tin_a < tout_v; }

inline bool lca_tree_ok(int64_t n_nodes, const int32_t* parent) {
  if (n_nodes < 1 || n_nodes > INT32_MAX || !parent || parent[0] != 0) return false;
  for (int64_t v = 1; v < n_nodes; ++v) if (parent[v] < 0 || parent[v] >= v) return false;
  return true;
}
inline bool lca_taxa_ok(int64_t n_taxa, const int32_t* taxon_node, int64_t n_nodes) {
  if (!taxon_node) return false;
  for (int64_t t = 0; t < n_taxa; ++t) if (taxon_node[t] < 0 || taxon_node[t] >= n_nodes) return false;
  return true;
}
// depth (may be null), tin and tout of a tree that lca_tree_ok accepts, children in index order.  tout[v] holds the size of v's subtree until
// v gets its tin, then the tin of v's next child: tin[v] + size once every child has been placed.
inline void lca_derive(int64_t n_nodes, const int32_t* parent, int32_t* depth, int32_t* tin, int32_t* tout) {
  for (int64_t v = 0; v < n_nodes; ++v) tout[v] = 1;
  for (int64_t v = n_nodes - 1; v > 0; --v) tout[parent[v]] += tout[v];
  tin[0] = 0; tout[0] = 1;
  if (depth) depth[0] = 0;
  for (int64_t v = 1; v < n_nodes; ++v) {
    const int32_t p = parent[v], size = tout[v];
    tin[v] = tout[p]; tout[p] += size; tout[v] = tin[v] + 1;
    if (depth) depth[v] = depth[p] + 1;
  }
}

struct LcaTree { const int32_t* tin; const int32_t* tout; const int32_t* parent; };

// the lanes that share a read: lane l of `width` takes the entries l, l + width, ...; sum / min / max / any give every lane the same value
struct LcaSerial {
  MM_HD int lane() const { return 0; }
  MM_HD int width() const { return 1; }
  MM_HD double sum(double x) const { return x; }
  MM_HD int32_t min(int32_t x) const { return x; }
  MM_HD int32_t max(int32_t x) const { return x; }
  MM_HD bool any(bool b) const { return b; }
};
// the entries of a read held in arrays: node and posterior of entry k
struct LcaArrayEntries {
  const int32_t* node_; const double* p_; const int32_t* tin_;
  MM_HD int32_t node(int64_t k) const { return node_[k]; }
  MM_HD int32_t tin(int64_t k) const { return tin_[node_[k]]; }
  MM_HD double p(int64_t k) const { return p_[k]; }
};

// lca(r) and *mass = mass(r, lca(r)) of a read of n entries; -1 and 0 for n == 0.  Every lane of `g` calls it (lanes of other reads of the
// wavefront too: `any` keeps the loops of all of them in step) and every lane of a read gets the result.
template <class G, class E> MM_HD int32_t lca_read(const G& g, const E& e, int64_t n, const LcaTree& T, double tau, double* mass) {
  double s = 0; int32_t lo = INT32_MAX, hi = -1;
  for (int64_t k = g.lane(); k < n; k += g.width()) { s += e.p(k); const int32_t t = e.tin(k); lo = t < lo ? t : lo; hi = t > hi ? t : hi; }
  const double total = g.sum(s);
  lo = g.min(lo); hi = g.max(hi);
  const bool live = n > 0 && lca_qualifies(total, tau);            // else: the root (rounding only), or no read
  if (!live) lo = hi = 0;
  const double half = 0.5 * total;
  bool bisect = lo < hi;
  while (g.any(bisect)) {                                          // invariant: mass(tin <= hi) >= half
    const int32_t mid = lo + (hi - lo) / 2;
    double c = 0;
    for (int64_t k = g.lane(); k < n; k += g.width()) if (e.tin(k) <= mid) c += e.p(k);
    c = g.sum(c);
    if (bisect) { if (c >= half) hi = mid; else lo = mid + 1; bisect = lo < hi; }
  }
  int32_t u = INT32_MAX;                                           // the node with tin == lo: an entry's (the sums change only there)
  for (int64_t k = g.lane(); k < n; k += g.width()) if (e.tin(k) == lo) { const int32_t v = e.node(k); u = v < u ? v : u; }
  u = g.min(u);
  if (!live) u = 0;
  double m = total;
  bool climb = live;
  while (g.any(climb)) {
    const int32_t a = T.tin[u], b = T.tout[u];
    double c = 0;
    for (int64_t k = g.lane(); k < n; k += g.width()) if (lca_in_subtree(e.tin(k), a, b)) c += e.p(k);
    c = g.sum(c);
    if (climb) { if (u == 0 || lca_qualifies(c, tau)) { m = c; climb = false; } else u = T.parent[u]; }
  }
  *mass = n > 0 ? m : 0.0;
  return n > 0 ? u : -1;
}

}  // namespace mm
