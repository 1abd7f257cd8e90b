// Confidence-thresholded lowest-common-ancestor assignment of every read of an EM problem (not in the reference; DESIGN.md section 4, "LCA
// assignment"): lca(r) = the deepest taxonomy node whose subtree holds at least tau of the read's posterior mass.  The per-read routine is
// mm_lca_core.hpp's lca_read — passes over the read's entries that are sums, minima and maxima — run here by two kinds of lanes:
//   short reads (<= LCA_GROUP = 16 entries; the rule)  four consecutive reads per wavefront, a group of 16 lanes each, one lane per entry: node,
//                tin and posterior of the entry stay in registers, every pass is a butterfly over the group;
//   long reads   (repeat-rich samples: thousands of entries) the whole wavefront strides over the read's entries, pass after pass; the
//                entries come from memory again (the loads hit the cache), the reductions are butterflies over 64 lanes.
// Both classes of a tile of four reads are handled by the wavefront that owns the tile (the loop over the tiles and the lanes' butterflies:
// mm_prims.hpp, for_each_read_tile and Lanes<W>; the kernel hands it the two routines); the loops of lca_read run while ANY lane of the
// wavefront needs them (groups that are done idle), so every shuffle is executed by all 64 lanes.  A sum that is exact in double is the same
// in either shape, so the split point does not change such results.
// tin / tout / parent of the tree lie in LDS when it has at most LCA_LDS_NODES nodes (the per-entry lookups tin[node] are gathers), else in
// global memory.  direct[v] counts the reads assigned to v with 64-bit vector atomics.  All entry and read indices are 64-bit.
#include "mm_lca.hpp"
#include "mm_prims.hpp"
#include <algorithm>

namespace mm {

struct LcaOwnEntry {                                              // the one entry of this lane
  int32_t node_, tin_; double p_;
  __device__ int32_t node(int64_t) const { return node_; }
  __device__ int32_t tin(int64_t) const { return tin_; }
  __device__ double p(int64_t) const { return p_; }
};
struct LcaReadEntries {                                           // entry k of the read whose entries begin at lo
  const int32_t* taxon; const double* post; const int32_t* taxon_node; const int32_t* tin_; int64_t lo;
  __device__ int32_t node(int64_t k) const { return taxon_node[taxon[lo + k]]; }
  __device__ int32_t tin(int64_t k) const { return tin_[node(k)]; }
  __device__ double p(int64_t k) const { return post[lo + k]; }
};

struct LcaArgs {
  const int64_t* read_off; const int32_t* taxon; const double* post; int64_t n_reads;
  const int32_t* taxon_node; LcaTree tree; int32_t n_nodes; double tau;
  int32_t* node_out; double* mass_out; unsigned long long* direct;   // mass_out, direct: may be null
};

__device__ inline void lca_store(const LcaArgs& a, int64_t r, int32_t v, double m) {
  a.node_out[r] = v;
  if (a.mass_out) a.mass_out[r] = m;
  if (a.direct && v >= 0) atomicAdd(&a.direct[v], 1ull);
}

template <bool IN_LDS> __global__ void __launch_bounds__(256) lca_assign_kernel(LcaArgs a) {
  extern __shared__ __align__(16) int32_t lca_sh[];
  LcaTree T = a.tree;
  if (IN_LDS) {
    const int n = a.n_nodes;
    for (int i = threadIdx.x; i < n; i += 256) { lca_sh[i] = a.tree.tin[i]; lca_sh[n + i] = a.tree.tout[i]; lca_sh[2 * n + i] = a.tree.parent[i]; }
    __syncthreads();
    T = LcaTree{lca_sh, lca_sh + n, lca_sh + 2 * n};
  }
  for_each_read_tile<LCA_GROUP>(a.read_off, a.n_reads,
    [&](int64_t r, int64_t lo, int64_t n, bool mine, int gl) {    // the tile's short reads, and its reads without entries
      LcaOwnEntry e{0, 0, 0.0};
      if (mine && gl < n) { e.node_ = a.taxon_node[a.taxon[lo + gl]]; e.tin_ = T.tin[e.node_]; e.p_ = a.post[lo + gl]; }
      double m;
      const int32_t v = lca_read(Lanes<LCA_GROUP>{}, e, mine ? n : 0, T, a.tau, &m);
      if (mine && gl == 0) lca_store(a, r, v, m);
    },
    [&](int64_t r, int64_t lo, int64_t n) {                       // its long reads, one after the other
      double m;
      const int32_t v = lca_read(Lanes<64>{}, LcaReadEntries{a.taxon, a.post, a.taxon_node, T.tin, lo}, n, T, a.tau, &m);
      if (Lanes<64>{}.lane() == 0) lca_store(a, r, v, m);
    });
}

void lca_run(mm_em* E, const double* f, int32_t n_nodes, const int32_t* parent, const int32_t* taxon_node, double tau,
             int32_t* node_out, double* mass_out, int64_t* direct_out) {
  MM_REQUIRE(lca_threshold_ok(tau), MM_ERR_ARG, "LCA threshold outside [0.51, 1]");
  MM_REQUIRE(lca_tree_ok(n_nodes, parent), MM_ERR_ARG, "LCA tree: parent[0] must be 0 and 0 <= parent[v] < v for v > 0");
  MM_REQUIRE(lca_taxa_ok(E->n_taxa, taxon_node, n_nodes), MM_ERR_ARG, "LCA tree: a taxon's node lies outside the tree");
  hipStream_t st = E->ctx->stream;
  const size_t N = (size_t)n_nodes, NR = (size_t)E->n_reads;
  std::vector<int32_t> tree(3 * N);                                // tin | tout | parent
  lca_derive(n_nodes, parent, nullptr, tree.data(), tree.data() + N);
  std::copy(parent, parent + N, tree.begin() + 2 * (long)N);
  DBuf<int32_t> d_tree(3 * N), d_tn((size_t)E->n_taxa), d_node(std::max<size_t>(NR, 1));
  DBuf<double> d_mass; DBuf<unsigned long long> d_direct;
  d_tree.upload(tree.data(), tree.size(), st);
  d_tn.upload(taxon_node, (size_t)E->n_taxa, st);
  if (mass_out) d_mass.alloc(std::max<size_t>(NR, 1));
  if (direct_out) { d_direct.alloc(N); d_direct.zero(st); }
  em_estep(E, f);
  if (NR > 0) {
    LcaArgs a{E->read_off.p, E->taxon.p, E->post.p, E->n_reads, d_tn.p, LcaTree{d_tree.p, d_tree.p + N, d_tree.p + 2 * N}, n_nodes, tau,
              d_node.p, d_mass.p, d_direct.p};
    const dim3 grid(read_tile_grid<LCA_GROUP>(E->n_reads)), blk(256);
    if (n_nodes <= LCA_LDS_NODES) lca_assign_kernel<true><<<grid, blk, 3 * N * sizeof(int32_t), st>>>(a);
    else lca_assign_kernel<false><<<grid, blk, 0, st>>>(a);
    MM_KERNEL_CHECK();
  }
  d_node.download(node_out, NR, st);
  if (mass_out) d_mass.download(mass_out, NR, st);
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "direct_out is copied as it lies");
  if (direct_out) d_direct.download((unsigned long long*)direct_out, N, st);
  MM_HIP(mm::stream_sync(st));
}

}  // namespace mm
