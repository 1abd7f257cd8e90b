// Per-batch mapping pipeline on the device (replaces Map::mapModule → mapSingleQuerySeq → doL1Mapping /
// doL2Mapping, computeMap.hpp:180-538, for a whole batch of reads; output order == input order, which is
// all the reference's ThreadPool guarantees, ThreadPool.hpp:13-17).
//
//   K1  minimizer sweep of the reads                         mm_minimizer.hpp
//   K2  sketch = sort by hash + unique                       computeMap.hpp:292-298
//   K3  index probe + seed-hit gather                        computeMap.hpp:307-323
//   K4  hit sort + L1 candidate scan                         computeMap.hpp:346-386
//   K5  L2 sliding MinHash window + K6 strand vote           computeMap.hpp:460-538, slidingMap.hpp
//   K7  identity filter: a per-sketch-size integer threshold computed on the host (mm_stats.hpp)
#include "mm_map.hpp"
#include <functional>
#include <memory>
#include "mm_prims.hpp"
#include "mm_l2_core.hpp"
#include "mm_size_classes.hpp"
#include "mm_l2.hpp"
#include "mm_l2z.hpp"
#include "mm_l2_dense.hpp"
#include <cstdlib>
#include <atomic>
#include <thread>
#include "mm_stats.hpp"
#include <algorithm>
#include <numeric>
#include "mm_sketch.hpp"
#include "mm_seed.hpp"
#include "mm_l1.hpp"

namespace mm {

// ---------------------------------------------------------------------------------------------------
// host orchestration
// ---------------------------------------------------------------------------------------------------
namespace {
// MM_HOST_TIMING=1: wall time of the host sections between kernels (stderr)
struct HostLap {
  const bool on = getenv("MM_HOST_TIMING") != nullptr; std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void operator()(const char* what) { if (!on) return; const auto n = std::chrono::steady_clock::now(); fprintf(stderr, "host %-28s %8.1f us\n", what, std::chrono::duration<double, std::micro>(n - t).count()); t = n; }
};

// Reads grouped by a small class id (n_classes: left out), input order kept inside a class: a counting sort without data-dependent
// branches, because these host loops sit between two kernels of a batch with the device waiting (std::map + push_back, or a branchy
// class function on mixed counts, cost ~0.6 ms per 10^5 reads in mispredictions).
struct ReadBins { std::vector<int32_t> order; std::vector<std::pair<int, size_t>> runs; };   // runs: (class, number of reads), ascending class, back to back in `order`
template <typename F>
ReadBins bin_reads(int64_t n, int n_classes, F&& class_of) {
  ReadBins b;
  std::vector<size_t> start((size_t)n_classes + 2, 0);
  std::vector<uint8_t> cls((size_t)std::max<int64_t>(n, 0));
  for (int64_t r = 0; r < n; ++r) { const unsigned c = (unsigned)class_of(r); cls[(size_t)r] = (uint8_t)c; ++start[(size_t)c + 1]; }
  for (int c = 0; c <= n_classes; ++c) start[(size_t)c + 1] += start[(size_t)c];
  b.order.resize((size_t)std::max<int64_t>(n, 0));               // the left-out reads land behind the classes and are cut off
  std::vector<size_t> at(start.begin(), start.end() - 1);
  for (int64_t r = 0; r < n; ++r) b.order[at[cls[(size_t)r]]++] = (int32_t)r;
  b.order.resize(start[(size_t)n_classes]);
  for (int c = 0; c < n_classes; ++c) if (start[(size_t)c + 1] > start[(size_t)c]) b.runs.emplace_back(c, start[(size_t)c + 1] - start[(size_t)c]);
  return b;
}

struct HostMz { uint32_t hash; int32_t wpos, strand; };
static bool host_less_by_hash(const HostMz& a, const HostMz& b) { return a.hash < b.hash; }   // base_types.hpp:70
static bool host_eq_by_hash(const HostMz& a, const HostMz& b) { return a.hash == b.hash; }    // base_types.hpp:66
}  // namespace

namespace {
// hipEvent pairs on the ctx stream; elapsed times are read once at the end of the batch
struct StageTimer {
  hipStream_t st;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  std::vector<double*> dst;
  explicit StageTimer(hipStream_t s) : st(s) {}
  ~StageTimer() { for (auto& e : ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); } }
  size_t begin(double* target) {
    hipEvent_t a, b;
    MM_HIP(hipEventCreate(&a)); MM_HIP(hipEventCreate(&b));
    ev.push_back({a, b}); dst.push_back(target);
    MM_HIP(hipEventRecord(a, st));
    return ev.size() - 1;
  }
  void end(size_t i) { MM_HIP(hipEventRecord(ev[i].second, st)); }
  void collect() {
    MM_HIP(mm::stream_sync(st));
    for (size_t i = 0; i < ev.size(); ++i) { float ms = 0; MM_HIP(hipEventElapsedTime(&ms, ev[i].first, ev[i].second)); *dst[i] += ms; }
  }
};
}  // namespace

// one host-side duplicate-hash tie-break in flight (owned by MapRun::amb_states, never by its worker thread).  The worker sees a raw
// pointer to this struct and nothing else of the run, so all it needs is that the struct outlives it: the destructor joins first.  In
// MapRun, amb_states is declared behind amb_finish (whose closure points into it) and in front of the device buffers of the later
// stages, which therefore go back to the context's cache before the join, as they did when all of these were locals of map_batch.
struct AmbState {
  std::thread bg;                          // (the destructor body joins it before any member is destroyed)
  std::vector<Rec> hr; std::vector<uint64_t> dof; std::vector<int32_t> expect; DBuf<uint64_t> d_so, d_do;
  std::vector<uint8_t> sv; std::vector<int32_t> scnt; std::atomic<int> mismatch{0};
  ~AmbState() { if (bg.joinable()) bg.join(); }
};

namespace {
// Every MM_* switch map_batch reads (mm_env.hpp), each read once at the start of a call.  Never cached in a static or per context: tests
// set and clear them between two calls of one process, and a switch takes effect at the next call.
struct MapSwitches {
  struct OptInt { bool set; int v; };
  static bool on(const char* e) { return e != nullptr; }
  static bool is1(const char* e) { return e && e[0] == '1'; }
  static int num(const char* e, int dflt) { return e ? atoi(e) : dflt; }
  static OptInt opt(const char* e) { return OptInt{e != nullptr, e ? atoi(e) : 0}; }
  // K2
  const bool eager_tiebreak = on(getenv("MM_EAGER_TIEBREAK"));   // tests that compare every sketch strand with the oracle
  // K3
  const bool use_filter = !is1(getenv("MM_NO_HIT_FILTER"));      // parity tests of the raw hit list
  // the fused probe + filter kernel takes the reads whose sketch fits its LDS layout (MM_NO_FUSED_FILTER=1: cross-check switch)
  const bool use_fused = use_filter && !on(getenv("MM_NO_FUSED_FILTER"));
  // which kernel filters a read: 0 the fused kernel, 1 the two-pass kernels with 8 192 slots, 2 with 32 768 slots (sketches beyond
  // MM_HF_WIDE_FROM hashes, default 13000 = reads from ~58 kb on; 0 switches the wide table off).  Measured on the bench reference:
  // 45-58 kb reads 88.8 ms narrow / 91.2 ms wide per batch of 8 000 (the wide kernel reads 8-byte entries, three requests per list
  // instead of one, on one workgroup per CU), 60-73 kb reads 873 / 125 ms per batch of 6 000, 75-140 kb 1 388 / 376 ms per 4 000.
  const int hf_wide_env = num(getenv("MM_HF_WIDE_FROM"), 13000);
  const int hf_wide_from = hf_wide_env > 0 ? hf_wide_env : INT_MAX;
  const OptInt hf_stage_cap = opt(getenv("MM_HF_STAGE_CAP"));    // tests: a tiny capacity forces the re-filtering write path
  const int hf_dbg = num(getenv("MM_HF_DBG"), 0);
  // the fused kernel streams: one resident workgroup per CU, look-ups of the next read under the LDS phases of this one
  const bool sf_prof = on(getenv("MM_SF_PROF"));                 // cycles per phase of the streaming kernel, printed per batch
  const OptInt sf_grid = opt(getenv("MM_SF_GRID"));              // (measurement aid: fewer resident workgroups = fewer CUs at work)
  // K4
  // beyond 4096 hits a read takes the device's segmented radix sort, at most max_keys - 1 keys per call (test hook, small values: the split on small inputs)
  const OptInt segsort_max_env = opt(getenv("MM_SEGSORT_MAX_KEYS"));
  const uint64_t segsort_max_keys = segsort_max_env.set ? (uint64_t)std::max(segsort_max_env.v, 1) : 0xffffffffull;
  const bool l1_serial = on(getenv("MM_L1_SERIAL"));             // cross-check switch: the one-thread-per-read loop
  const bool l2_no_fuse = on(getenv("MM_L2_NO_FUSE"));           // no band prediction from the L1 kernel
  // K5
  const bool l2_no_ranges = on(getenv("MM_L2_NO_RANGES"));       // the zone kernel's waves search their ranges themselves, as until round 6
  const bool l2_skip = !is1(getenv("MM_L2_FULL"));               // MM_L2_FULL=1, cross-check switch: evaluate every window
  // sketches from this size on take the dense path (MM_L2_DENSE_FROM: experiments, tests)
  // (from ~58 kb reads on the streamed range of a candidate outgrows the 32 768-entry masks of the LDS classes' exact skip-ahead, which
  //  then evaluate every window with a rebuild per zone exit: 6 000 reads of 60-73 kb: 171 ms there, 83 ms here)
  const int dense_from = num(getenv("MM_L2_DENSE_FROM"), 13000);
  const bool dense_no_stop = on(getenv("MM_L2_DENSE_NO_STOP"));
  const bool no_small_groups = on(getenv("MM_L2_NO_SMALL_GROUPS"));   // cross-check / timing switch
  // the zone kernels (mm_l2z.hpp) run the classes of sketches up to 16 384 hashes.  MM_L2_V1=1: every candidate below L2_SKETCH_LIMIT that is not
  // on the dense path goes through l2_kernel's wide form instead, one wave per candidate (the zone kernels' cross-check)
  const bool v2 = !on(getenv("MM_L2_V1"));
  const bool v2_long = v2 && !on(getenv("MM_L2_V1_LONG"));       // (MM_L2_V1_LONG=1: only the long-read classes B and D go that way)
  // the workgroups of the 10 kb class are put together on the device while the L1 kernel still runs (l2_group_kernel);
  // MM_L2_HOST_GROUPS=1: the host loop makes them as well (cross-check)
  const bool dev_groups = l2_skip && v2 && !on(getenv("MM_L2_HOST_GROUPS"));
  // scratch slots of the skip kernels (mm_l2.hpp): a slot per RESIDENT wave (the hardware keeps at most 32 per CU), taken and given
  // back by the waves through one flag word each; MM_L2_NO_SLOTS=1: one slot per wave of the launch, no flags (cross-check switch)
  // (MM_L2_SLOTS=n, rounded up to a multiple of 8: fewer slots than resident waves — they wait for each other's; tests of the hand-over)
  const bool l2_no_slots = on(getenv("MM_L2_NO_SLOTS"));
  const OptInt l2_slots_env = opt(getenv("MM_L2_SLOTS"));
  const size_t l2_slots = l2_slots_env.set ? ((size_t)std::max(l2_slots_env.v, 1) + 7) / 8 * 8 : 0;
  const bool sort_groups = !on(getenv("MM_L2_NO_GROUP_SORT"));
  const OptInt group_sort_env = opt(getenv("MM_L2_GROUP_SORT_MIN"));   // (test hook: small batches take the sort too)
  const size_t group_sort_from = group_sort_env.set ? (size_t)std::max(group_sort_env.v, 1) : 2048;
  const bool one_stream = on(getenv("MM_L2_ONE_STREAM"));        // the two launches of the 10 kb class one behind the other as until round 5 (cross-check and A/B)
  // the debug word of the K5 kernels (counters[11])
  const OptInt l2_stop = opt(getenv("MM_L2_STOP"));              // timing aid: leave the kernel after phase n (results are then meaningless)
  const bool l2_phases = on(getenv("MM_L2_PHASES"));
  const bool force_amb_redo = on(getenv("MM_FORCE_AMB_REDO"));
  const OptInt l2z_dbg = opt(getenv("MM_L2Z_DBG"));
  const bool l2z_force_handback = on(getenv("MM_L2Z_FORCE_HANDBACK"));
  const bool l2z_walk_search = on(getenv("MM_L2Z_WALK_SEARCH"));
  bool has_l2_debug_word() const { return l2_stop.set || l2_phases || force_amb_redo || l2z_dbg.set || l2z_force_handback || l2z_walk_search; }
  unsigned long long l2_debug_word() const {
    int v = l2_stop.set ? l2_stop.v & 0xff : 0;
    if (l2_phases) v |= 0x100;
    if (force_amb_redo) v |= 0x200;
    if (l2z_dbg.set) v |= l2z_dbg.v == 2 ? 0xc00 : 0x400;
    if (l2z_force_handback) v |= 0x1000;
    if (l2z_walk_search) v |= 0x2000;
    return (unsigned long long)v;
  }
};

// a run-time items-per-thread value -> f(std::integral_constant<int, IPT>) for the value of the list it equals (the last one takes the rest)
template <int First, int... Rest, typename F>
void dispatch(int ipt, F&& f) {
  if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<int, First>{});
  else if (ipt == First) f(std::integral_constant<int, First>{});
  else dispatch<Rest...>(ipt, f);
}

void set_lds(const void* fn, size_t bytes) { if (bytes > 64 * 1024) MM_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes)); }

// One call of map_batch: what crosses a stage boundary, one method per stage.  The members are declared in the order the locals of the one
// long function were, so the device buffers go back to the context's cache in the same order on every way out.
struct MapRun {
  mm_ctx* const ctx; const mm_index* const I; const mm_seqset* const reads; const mm_map_params& P; mm_mapping* const M;
  const hipStream_t st;
  const MapSwitches sw;
  StageTimer T;
  const int64_t n;
  size_t t_total = 0, t_l1 = 0;
  int64_t total_mz = 0, total_hits = 0, ncand = 0;
  HostLap hl;
  std::vector<uint8_t> h_amb;
  std::function<void()> amb_finish;                              // joins the eager tie-break and patches the strands: called right before the first L2 launch
  std::vector<int64_t> eager_reads, lazy_reads;
  // The tie-break states live here: whatever way map_batch is left (return, MM_REQUIRE, a failed allocation), their
  // destructors join the worker first and release the device buffers on this thread.  The worker only sees a raw pointer and
  // its own copies of the host data it reads.
  std::vector<std::unique_ptr<AmbState>> amb_states;
  IndexView IV{};
  // K3 .. K4b
  DBuf<uint32_t> probe_cnt;
  DBuf<uint64_t> probe_start;
  DBuf<uint64_t> hit_off, scan_tmp;
  DBuf<uint8_t> need_old; DBuf<uint32_t> raw_per_read;
  int64_t n_fused = 0, n_wide = 0;
  uint64_t raw_hits = 0;                                         // (target of an async download: read after the wait for the hit offsets)
  DBuf<unsigned long long> raw_sum;
  DBuf<uint32_t> surv;
  DBuf<uint64_t> stage, stage_off;
  const uint8_t* only = nullptr;                                 // the class bytes of the filter path: the two-pass kernels skip what the fused kernel took
  DBuf<uint32_t> cand_n;
  DBuf<int32_t> cand_hint;                                       // seed hits inside each candidate (l1_wave_kernel): the zone kernel's prediction of its band
  DBuf<int64_t> cand_rng;                                        // [first, behind-last) index entry of each candidate's stream (l2_ranges_kernel)
  // K5, to the end of the batch
  DBuf<int32_t> d_gA0, d_gAn, d_gS0, d_gSn;                      // four-wave and two-wave groups of the 10 kb class
  DBuf<unsigned int> grp_ctr;
  std::vector<int32_t> listG; int smG = 0;                       // candidates of sketches of >= L2_SKETCH_LIMIT hashes
  DBuf<unsigned long long> counters;
  DBuf<int32_t> ovf;
  DBuf<unsigned int> ovf_n;
  DBuf<uint8_t> amb_used;
  uint8_t* amb_used_p = nullptr;
  // K5, the skip classes only: released by l2_skip_classes where its block ended, in front of the compaction's allocations
  struct SkipClasses {
    DBuf<unsigned int> slot_flags;
    DBuf<int32_t> big;                                           // candidates with more streamed entries than the zone kernel's masks hold: l2_kernel's wide form
    DBuf<unsigned int> big_n;
    std::vector<int32_t> gA0, gAn, gB0, gBn, gD0, gDn, listC, gS0, gSn;   // gS: groups of one or two candidates of the 10 kb class (two-wave workgroups)
    int smA = 0, smB = 0, smC = 0, smD = 0;
    std::vector<int32_t> listL; int smL = 0;                     // long reads below the giant class that take the dense path
    std::vector<unsigned int> gctr = std::vector<unsigned int>(4, 0);
    size_t nA = 0, nS = 0;
    DBuf<int32_t> d_gB0, d_gBn, d_listC, d_gD0, d_gDn;
    int64_t n_fallback = 0, n_big = 0, n_redo = 0;
  };
  std::unique_ptr<SkipClasses> sk;

  MapRun(mm_ctx* ctx_, const mm_index* I_, const mm_seqset* reads_, const mm_map_params& P_, mm_mapping* M_)
      : ctx(ctx_), I(I_), reads(reads_), P(P_), M(M_), st(ctx_->stream), T(st), n(reads_->count()) {}

  const std::vector<uint64_t>& hoff() const { return M->mz.h_off; }
  int min_mapped_len() const { return P.w + P.k + 1; }           // shorter reads are handed back by the skip kernels
  bool dense_read(int64_t r, int sr) const { return sr >= sw.dense_from && sr < L2_SKETCH_LIMIT && M->read_len[(size_t)r] >= min_mapped_len(); }
  bool filtering() const { return sw.use_filter && n > 0; }

  void begin() {
    MM_REQUIRE(M->sketch_only || (I && I->k == P.k && I->w == P.w), MM_ERR_ARG, "index was built with different k / window size");   // (mm_sketch_batch: no index)
    MM_REQUIRE(n < (1LL << 31), MM_ERR_LIMIT, "more than 2^31 reads in one batch");
    M->ctx = ctx; M->n_reads = n; M->params = P; M->stats = mm_map_stats{};
    M->stats.n_reads = n;
    M->read_len = reads->len;
    M->active.assign((size_t)n, 0);
    for (int64_t r = 0; r < n; ++r) {
      int L = reads->len[(size_t)r];
      bool ok = !(L < P.w || L < P.k || L < P.min_read_len);      // computeMap.hpp:137
      M->active[(size_t)r] = ok;
      if (ok) { M->stats.n_reads_long_enough++; M->stats.bases_long_enough += L; }
    }
    t_total = T.begin(&M->stats.ms_total);
  }

  // ---- K1
  // The minimizers and the sketch of a read do not depend on the index: when the same batch is mapped against one index chunk after
  // the other (--maxmemory; the reference runs the whole of mapSingleQuerySeq per chunk, computeMap.hpp:277-298 included), the second
  // and later mappings take them from the first (mm_map_batch_reusing: the two large arrays held jointly, the rest copied).  Strands the donor's tie-break has resolved meanwhile are the
  // strands this mapping would resolve them to (the same library calls on the same records).
  void minimizers() {
    const mm_mapping* const donor = M->sketch_donor;
    if (donor) {
      const size_t t = T.begin(&M->stats.ms_minimizer);
      auto dcopy = [&](auto& dst, const auto& src) { dst.alloc(src.n); if (src.n) MM_HIP(hipMemcpyAsync(dst.p, src.p, src.bytes(), hipMemcpyDeviceToDevice, st)); };
      // the two big read-only arrays — minimizer records (8 B per minimizer) and sketch hashes (4 B) — are held jointly with the donor, not
      // copied (2.2 GB per chunk mapping of a 0.8 Gbp batch); the strand bytes and the per-read arrays are this mapping's own (its tie-break
      // writes to them)
      mm_mapping* const dn = const_cast<mm_mapping*>(donor);       // (only the ownership record of the two blocks changes)
      const bool same_ctx = donor->ctx == ctx;                     // (a block shared across contexts could go back to one context's cache while the other's stream still reads it)
      if (same_ctx) M->mz.rec.share_from(dn->mz.rec); else dcopy(M->mz.rec, donor->mz.rec);
      dcopy(M->mz.off, donor->mz.off);
      M->mz.h_off = donor->mz.h_off; M->mz.total = donor->mz.total;
      if (same_ctx) M->sk_hash.share_from(dn->sk_hash); else dcopy(M->sk_hash, donor->sk_hash);
      dcopy(M->sk_strand, donor->sk_strand); dcopy(M->sk_n, donor->sk_n); dcopy(M->amb, donor->amb);
      T.end(t);
    } else { size_t t = T.begin(&M->stats.ms_minimizer); run_minimizers(ctx, reads, P.k, P.w, M->active, false, M->mz); T.end(t); }
    total_mz = M->mz.total;
    if (!donor) {
      M->sk_hash.alloc((size_t)std::max<int64_t>(total_mz, 1));
      M->sk_strand.alloc((size_t)std::max<int64_t>(total_mz, 1));
      M->sk_n.alloc((size_t)std::max<int64_t>(n, 1)); M->sk_n.zero(st);
      M->amb.alloc((size_t)std::max<int64_t>(n, 1)); M->amb.zero(st);
    }
  }

  // ---- K2 (a donor's sketches are this mapping's already)
  void sketch() {
    if (M->sketch_donor) return;
    size_t t_sk = T.begin(&M->stats.ms_sketch);
    // up to 16384 minimizers: radix sort in LDS, 4 ... 64 elements per thread.  The sort's cost follows the elements per thread, so the
    // reads are grouped by the capacity they really need (a 10 kb read has ~2 200 minimizers: 10 per thread instead of 16).
    // Single-element lists are "sorted" already but still need their sketch written.
    static_assert(ipt_list_is<4, 6, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64>(SKETCH_IPTS), "the dispatch below lists the classes of mm_size_classes.hpp");
    uint64_t big_seen = 0;
    HostLap hl;
    const ReadBins RB = bin_reads(n, N_SKETCH_CLASSES, [&](int64_t r) -> int {
      const uint64_t c = hoff()[(size_t)r + 1] - hoff()[(size_t)r];
      big_seen |= (uint64_t)(c > SKETCH_LDS_MAX);
      return sketch_class_index(c);                                // (empty reads and those beyond the LDS sort are left out)
    });
    const bool any_big = big_seen != 0;
    {
      hl("K2 bin");
      DBuf<int32_t> list(std::max<size_t>(RB.order.size(), 1));
      list.upload(RB.order.data(), RB.order.size(), st);
      hl("K2 list upload");
      size_t at = 0;
      for (auto& run : RB.runs) {
        const unsigned nb = (unsigned)run.second;
        const int32_t* lp = list.p + at;
        dispatch<4, 6, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64>(SKETCH_IPTS[run.first], [&](auto ipt_tag) {
          constexpr int IPT = decltype(ipt_tag)::value;
          using SortT = rocprim::block_radix_sort<uint32_t, 256, IPT, uint16_t>;
          using ScanT = rocprim::block_scan<int, 256>;
          const size_t lds = std::max(sizeof(typename SortT::storage_type), sizeof(typename ScanT::storage_type)) + 16;
          if (lds > 48 * 1024) MM_HIP(hipFuncSetAttribute((const void*)sketch_radix_kernel<IPT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
          sketch_radix_kernel<IPT><<<dim3(nb), dim3(256), lds, st>>>(M->mz.rec.p, M->mz.off.p, lp, M->sk_hash.p, M->sk_strand.p, M->sk_n.p, M->amb.p);
        });
        MM_KERNEL_CHECK();
        at += run.second;
      }
      hl("K2 launches");
      MM_HIP(mm::stream_sync(st));                          // RB.order is the source of the async upload
      hl("K2 sync (kernels)");
    }
    if (any_big) sketch_big_segmented();                          // longer lists (reads beyond ~73 kb)
    T.end(t_sk);
  }

  // sketches of the reads beyond 16 384 minimizers: keys of all of them back to back, one segmented device sort, unique + strand per read
  void sketch_big_segmented() {
    std::vector<int32_t> big; std::vector<uint64_t> koff{0};
    for (int64_t r = 0; r < n; ++r) { const uint64_t c = hoff()[(size_t)r + 1] - hoff()[(size_t)r]; if (c > SKETCH_LDS_MAX) { big.push_back((int32_t)r); koff.push_back(koff.back() + c); } }
    const size_t nb = big.size(); const uint64_t nk = koff.back();
    MM_REQUIRE(nk < ((uint64_t)1 << 32), MM_ERR_LIMIT, "more than 2^32 minimizers of reads beyond 16384 minimizers in one batch");
    DBuf<int32_t> d_big(nb); d_big.upload(big.data(), nb, st);
    DBuf<uint64_t> d_koff(nb + 1); d_koff.upload(koff.data(), nb + 1, st);
    DBuf<uint64_t> keys((size_t)nk), sorted((size_t)nk);
    sketch_keys_kernel<<<dim3((unsigned)nb), dim3(256), 0, st>>>(M->mz.rec.p, M->mz.off.p, d_big.p, d_koff.p, keys.p);
    MM_KERNEL_CHECK();
    DBuf<uint8_t> tmp;
    with_scratch(tmp, [&](void* t, size_t& b) { return rocprim::segmented_radix_sort_keys(t, b, keys.p, sorted.p, (unsigned int)nk, (unsigned int)nb, d_koff.p, d_koff.p + 1, 0, 64, st); });
    sketch_finish_kernel<<<dim3((unsigned)nb), dim3(256), 0, st>>>(M->mz.rec.p, M->mz.off.p, d_big.p, d_koff.p, sorted.p, M->sk_hash.p, M->sk_strand.p, M->sk_n.p, M->amb.p);
    MM_KERNEL_CHECK();
    MM_HIP(mm::stream_sync(st));                          // big / koff are upload sources
  }

  // false: mm_sketch_batch (K1 + K2 alone, the donor of mm_map_batch_reusing), the mapping is complete
  bool after_sketch() {
    hl.t = std::chrono::steady_clock::now();
    M->h_sk_n = M->sk_n.to_host(st, (size_t)n);
    if (M->sketch_only) {
      for (int64_t r = 0; r < n; ++r) M->stats.sum_sketch += M->h_sk_n[(size_t)r];
      M->h_rec_off.assign((size_t)n + 1, 0); M->n_rec = 0;          // an empty mapping for every call that reads records
      T.end(t_total);
      T.collect();
      return false;
    }
    // mm_map_batch_phased, stage 1: K1 + K2 are complete (the download above waited for them), nothing of the seed stage is enqueued yet
    if (M->at_stage) M->at_stage(M->at_stage_user, 1);
    h_amb = M->amb.to_host(st, (size_t)n);
    hl("post-K2 downloads");
    // Reads whose sketch has >= 32768 hashes (~145 kb at w = 8) are beyond the LDS-resident window state of the K5 classes
    // whatever MM_L2_DENSE_FROM says: their candidates always take the dense path; counted for the caller's information only.
    int64_t giant = 0;
    for (int64_t r = 0; r < n; ++r) if (M->h_sk_n[(size_t)r] >= L2_SKETCH_LIMIT) ++giant;
    M->stats.n_reads_giant = giant;
    return true;
  }

  // ---- duplicate-hash strand tie-break (computeMap.hpp:292-295: std::sort is not stable, std::unique keeps
  //      whichever equal-hash element introsort left first).  Only the strand of the survivor is observable
  //      (slidingMap.hpp:247), so it is resolved here with the same library calls on the same input order.
  //      Entries whose strand depends on that are marked by K2 (bit 1 of the strand byte); the library sort is only run for
  //      reads whose strand vote actually read such an entry (found out by K6, amb_used[]), and those few candidates are
  //      then redone.  MM_EAGER_TIEBREAK: every marked read is resolved up front.
  void tiebreak_lists() {
    for (int64_t r = 0; r < n; ++r) if (h_amb[(size_t)r]) (sw.eager_tiebreak ? eager_reads : lazy_reads).push_back(r);
    M->stats.n_ambiguous_sketch_reads = (int64_t)(eager_reads.size() + lazy_reads.size());
    hl("post-K2 amb lists");
    if (!eager_reads.empty()) amb_finish = start_tiebreak(eager_reads);
    hl("post-K2 tiebreak start");
  }

  // starts the host work for `amb_reads` on background threads and returns the closure that joins it and patches the strands
  std::function<void()> start_tiebreak(const std::vector<int64_t>& amb_reads) {
    const size_t na = amb_reads.size();
    std::vector<uint64_t> so(na), dof(na + 1, 0);
    std::vector<int32_t> expect(na);
    for (size_t i = 0; i < na; ++i) {
      int64_t r = amb_reads[i];
      so[i] = hoff()[(size_t)r];
      dof[i + 1] = dof[i] + (hoff()[(size_t)r + 1] - hoff()[(size_t)r]);
      expect[i] = M->h_sk_n[(size_t)r];
    }
    DBuf<uint64_t> d_so(na), d_do(na + 1);
    d_so.upload(so.data(), na, st); d_do.upload(dof.data(), na + 1, st);
    DBuf<Rec> comp((size_t)dof[na]);
    gather_amb_kernel<<<dim3((unsigned)na), dim3(256), 0, st>>>(M->mz.rec.p, d_so.p, d_do.p, comp.p);
    MM_KERNEL_CHECK();
    // The library sort of ~1 % of the reads is the only per-read host work of a batch.  Only the L2 strand vote needs its
    // result, so it runs on host threads while the device goes through K3 and K4.
    amb_states.push_back(std::make_unique<AmbState>());
    AmbState* const A = amb_states.back().get();
    A->hr = comp.to_host(st);
    A->dof = dof; A->expect = std::move(expect); A->d_so = std::move(d_so); A->d_do = std::move(d_do);
    A->sv.assign((size_t)dof[na], 0);
    A->scnt.assign(na, 0);
    // host part (no device calls): starts now on its own threads; joined right before the L2 launch
    A->bg = std::thread([A, na]() {
      std::atomic<size_t> next{0};
      auto worker = [&]() {
        std::vector<HostMz> v;
        for (size_t i = next.fetch_add(1); i < na; i = next.fetch_add(1)) {
          const size_t cntr = (size_t)(A->dof[i + 1] - A->dof[i]);
          v.resize(cntr);
          for (size_t j = 0; j < cntr; ++j) { const Rec& x = A->hr[(size_t)A->dof[i] + j]; v[j] = HostMz{x.hash, pw_wpos(x.pw), pw_strand(x.pw)}; }
          std::sort(v.begin(), v.end(), host_less_by_hash);
          auto ue = std::unique(v.begin(), v.end(), host_eq_by_hash);
          const size_t sN = (size_t)(ue - v.begin());
          if ((int64_t)sN != A->expect[i]) A->mismatch = 1;
          for (size_t j = 0; j < sN; ++j) A->sv[(size_t)A->dof[i] + j] = v[j].strand == 1 ? 1 : 0;
          A->scnt[i] = (int32_t)sN;
        }
      };
      const unsigned nthr = std::max(1u, std::min(32u, std::min<unsigned>(mm::cpu_budget(), (unsigned)((na + 15) / 16))));
      std::vector<std::thread> pool;
      for (unsigned t = 1; t < nthr; ++t) pool.emplace_back(worker);
      worker();
      for (auto& t : pool) t.join();
    });
    return [M = M, A, na, st = st]() {
      if (A->bg.joinable()) A->bg.join();
      MM_REQUIRE(A->mismatch == 0, MM_ERR_DEVICE, "sketch size disagrees between device and host tie-break");
      DBuf<uint8_t> d_sv(A->sv.size()); d_sv.upload(A->sv.data(), A->sv.size(), st);
      DBuf<int32_t> d_cnt(na); d_cnt.upload(A->scnt.data(), na, st);
      scatter_strand_kernel<<<dim3((unsigned)na), dim3(256), 0, st>>>(d_sv.p, A->d_so.p, A->d_do.p, d_cnt.p, M->sk_strand.p);
      MM_KERNEL_CHECK();
      MM_HIP(mm::stream_sync(st));                          // host vectors above are the H2D sources
    };
  }
  void finish_tiebreak() { if (amb_finish) { amb_finish(); amb_finish = nullptr; } }

  // ---- K7 host thresholds per distinct sketch size
  void thresholds() {
    if (!ctx->lut_cache || ctx->lut_k != P.k || ctx->lut_pi != P.perc_identity) {
      ctx->lut_cache = stats::LutCache::for_params(P.k, P.perc_identity);
      ctx->lut_k = P.k; ctx->lut_pi = P.perc_identity;
    }
    stats::LutCache& lut = *static_cast<stats::LutCache*>(ctx->lut_cache.get());
    std::vector<int32_t> mh((size_t)n, 0), am((size_t)n, 0);
    int smax = 0, s_hi = 0;
    for (int64_t r = 0; r < n; ++r) s_hi = std::max(s_hi, (int)M->h_sk_n[(size_t)r]);
    std::vector<int32_t> slot((size_t)s_hi + 1, -1);             // sketch size -> place in `sizes`
    std::vector<int> sizes;
    for (int64_t r = 0; r < n; ++r) { const int s = M->h_sk_n[(size_t)r]; if (s > 0 && slot[(size_t)s] < 0) { slot[(size_t)s] = (int32_t)sizes.size(); sizes.push_back(s); } }
    const std::vector<stats::SketchLut> luts = lut.get_many(sizes);
    for (int64_t r = 0; r < n; ++r) {
      int s = M->h_sk_n[(size_t)r];
      if (s <= 0) continue;
      const stats::SketchLut L = luts[(size_t)slot[(size_t)s]];
      mh[(size_t)r] = L.min_hits; am[(size_t)r] = L.accept_min;
      if (s < L2_SKETCH_LIMIT) smax = std::max(smax, s);         // (LDS sizing of the K5 classes; larger sketches never enter them)
      M->stats.sum_sketch += s;
    }
    M->smax = smax;
    M->min_hits.alloc((size_t)std::max<int64_t>(n, 1)); M->min_hits.upload(mh.data(), (size_t)n, st);
    M->accept_min.alloc((size_t)std::max<int64_t>(n, 1)); M->accept_min.upload(am.data(), (size_t)n, st);
    M->h_min_hits = mh;
    MM_HIP(mm::stream_sync(st));
    hl("K7 thresholds + uploads");
    M->d_read_len.alloc((size_t)std::max<int64_t>(n, 1));
    M->d_read_len.upload(reads->len.data(), (size_t)n, st);
    IV = make_view(I);
  }

  // ---- K3
  void seed_hits() {
    probe_cnt.alloc((size_t)total_mz + 1);
    probe_start.alloc((size_t)total_mz + 1);
    if (filtering()) { raw_per_read.alloc((size_t)n); raw_per_read.zero(st); }
    else if (total_mz > 0) probe_cnt.zero(st);                     // (unfiltered path: the offsets come from a scan over every slot)
    if (filtering()) {
      std::vector<uint8_t> h_need((size_t)n, 0);
      for (int64_t r = 0; r < n; ++r) {
        const int sr = M->h_sk_n[(size_t)r];
        const uint8_t c = sr > sw.hf_wide_from ? 2 : ((sw.use_fused && sr <= SF_SMAX) ? 0 : 1);
        h_need[(size_t)r] = c; n_fused += c == 0; n_wide += c == 2;
      }
      need_old.alloc((size_t)n + 4); need_old.upload(h_need.data(), (size_t)n, st);   // (+4: the streaming seed filter reads the class bytes as whole words)
      MM_HIP(mm::stream_sync(st));                            // h_need is the source of the async upload
    }
    hl("K3 prep (need_old etc.)");
    const size_t t_pg = T.begin(&M->stats.ms_probe_gather);
    M->read_hit_off.alloc((size_t)n + 1);
    raw_sum.alloc(1);
    if (filtering()) seed_stage_and_fused();
    only = filtering() ? need_old.p : nullptr;
    if (n > 0 && total_mz > 0) {                                     // (reads the fused kernel flagged are only known on the device: the two-pass kernels always run and skip the rest)
      probe_kernel<<<dim3((unsigned)n), dim3(256), 0, st>>>(IV, M->sk_hash.p, M->mz.off.p, M->sk_n.p, probe_cnt.p, probe_start.p, only);
      MM_KERNEL_CHECK();
    }
    if (!filtering()) {
      hit_off.alloc((size_t)total_mz + 2);
      exclusive_scan_u32_u64(probe_cnt.p, total_mz, hit_off.p, scan_tmp, st);
      MM_HIP(hipMemcpyAsync(&raw_hits, hit_off.p + total_mz, sizeof raw_hits, hipMemcpyDeviceToHost, st));
    }
    if (filtering()) {
      const bool time_old = !(sw.use_fused && n_fused > 0);        // ms_hit_filter: the kernel that handles the bulk of the reads
      const size_t t_hf = time_old ? T.begin(&M->stats.ms_hit_filter) : 0;
      launch_hit_filter<false>(nullptr, nullptr, sw.hf_dbg, raw_per_read.p);
      if (time_old) T.end(t_hf);
      raw_sum.zero(st);                                            // only the total of the raw seed hits is needed
      sum_u32_kernel<<<dim3(256), dim3(256), 0, st>>>(raw_per_read.p, n, raw_sum.p);
      MM_KERNEL_CHECK();
      MM_HIP(hipMemcpyAsync(&raw_hits, raw_sum.p, sizeof raw_hits, hipMemcpyDeviceToHost, st));
      exclusive_scan_u32_u64(surv.p, n, M->read_hit_off.p, scan_tmp, st);
    } else {
      read_hit_bounds_kernel<<<dim3((unsigned)ceil_div(n + 1, 256)), dim3(256), 0, st>>>(M->mz.off.p, hit_off.p, n, M->read_hit_off.p);
      MM_KERNEL_CHECK();
    }
    hl("K3 launches");
    M->h_read_hit_off = M->read_hit_off.to_host(st);
    hl("K3 wait + hit_off download");
    total_hits = (int64_t)M->h_read_hit_off[(size_t)n];
    M->stats.sum_hits = (int64_t)raw_hits;
    M->stats.sum_hits_kept = total_hits;
    M->hits.alloc((size_t)std::max<int64_t>(total_hits, 1));
    if (total_hits > 0) {
      if (sw.use_filter) launch_hit_filter<true>(M->read_hit_off.p, M->hits.p, 100, nullptr);
      else {
        gather_hits_kernel<<<dim3((unsigned)n), dim3(256), 0, st>>>(IV, M->mz.off.p, M->sk_n.p, probe_cnt.p, probe_start.p, hit_off.p, M->hits.p);
        MM_KERNEL_CHECK();
      }
    }
    T.end(t_pg);
  }

  // the two-pass filter (count pass, or the pass that writes the hits): the narrow table for every read, the wide one when a read asks for it
  template <bool WRITE>
  void launch_hit_filter(const uint64_t* hit_off_p, uint64_t* hits_p, int dbg, uint32_t* raw_p) {
    using HfN = HitFilterCfg<HF_SLOT_BITS_NARROW>; using HfW = HitFilterCfg<HF_SLOT_BITS_WIDE>;
    hit_filter_kernel<WRITE, HF_SLOT_BITS_NARROW><<<dim3((unsigned)n), dim3(HfN::THREADS), HfN::LDS, st>>>(IV, M->mz.off.p, M->sk_n.p, probe_cnt.p, probe_start.p, M->d_read_len.p,
                                                                   M->min_hits.p, surv.p, hit_off_p, hits_p, stage.p, stage_off.p, dbg, only, raw_p);
    if (n_wide > 0) {
      MM_KERNEL_CHECK();
      MM_HIP(hipFuncSetAttribute((const void*)hit_filter_kernel<WRITE, HF_SLOT_BITS_WIDE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)HfW::LDS));
      hit_filter_kernel<WRITE, HF_SLOT_BITS_WIDE><<<dim3((unsigned)n), dim3(HfW::THREADS), HfW::LDS, st>>>(IV, M->mz.off.p, M->sk_n.p, probe_cnt.p, probe_start.p, M->d_read_len.p,
                                                                   M->min_hits.p, surv.p, hit_off_p, hits_p, stage.p, stage_off.p, dbg, only, raw_p);
    }
    MM_KERNEL_CHECK();
  }

  // the staging area of the survivors, and the fused probe + filter kernel over the reads of class 0
  void seed_stage_and_fused() {
    surv.alloc((size_t)n + 1); surv.zero(st);
    std::vector<uint64_t> h_stage_off((size_t)n + 1, 0);
    for (int64_t r = 0; r < n; ++r)
      h_stage_off[(size_t)r + 1] = h_stage_off[(size_t)r] + (M->h_sk_n[(size_t)r] > 0 ? (sw.hf_stage_cap.set ? (uint64_t)sw.hf_stage_cap.v : 1024 + 2 * (uint64_t)M->h_sk_n[(size_t)r]) : 0);
    stage_off.alloc((size_t)n + 1); stage_off.upload(h_stage_off.data(), h_stage_off.size(), st);
    stage.alloc((size_t)std::max<uint64_t>(h_stage_off[(size_t)n], 1));
    MM_HIP(mm::stream_sync(st));                            // h_stage_off is the source of the async upload
    hl("K3 stage_off loop + upload");
    if (!(sw.use_fused && n_fused > 0)) return;
    const size_t lds = sizeof(SeedFilterStreamLds);
    MM_HIP(hipFuncSetAttribute((const void*)seed_filter_stream_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    MM_HIP(hipFuncSetAttribute((const void*)seed_filter_stream_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    DBuf<uint32_t> sf_ticket(1);
    sf_ticket.zero(st);
    DBuf<unsigned long long> sf_prof;
    if (sw.sf_prof) { sf_prof.alloc(16); sf_prof.zero(st); }
    int sf_grid = (int)std::min<int64_t>(n, std::max(ctx->cus, 1));
    if (sw.sf_grid.set) sf_grid = std::max(1, std::min(sf_grid, sw.sf_grid.v));
    const size_t t_sf = T.begin(&M->stats.ms_hit_filter);
    if (sf_prof.p)
      seed_filter_stream_kernel<true><<<dim3((unsigned)sf_grid), dim3(SF_THREADS), lds, st>>>(IV, M->sk_hash.p, M->mz.off.p, M->sk_n.p, M->d_read_len.p, M->min_hits.p, surv.p, stage.p, stage_off.p,
                                                                         need_old.p, reinterpret_cast<const uint32_t*>(need_old.p), raw_per_read.p, (int)n, sf_ticket.p, sf_prof.p);
    else
      seed_filter_stream_kernel<false><<<dim3((unsigned)sf_grid), dim3(SF_THREADS), lds, st>>>(IV, M->sk_hash.p, M->mz.off.p, M->sk_n.p, M->d_read_len.p, M->min_hits.p, surv.p, stage.p, stage_off.p,
                                                                         need_old.p, reinterpret_cast<const uint32_t*>(need_old.p), raw_per_read.p, (int)n, sf_ticket.p, nullptr);
    MM_KERNEL_CHECK();
    T.end(t_sf);
    if (sf_prof.p) {
      auto h = sf_prof.to_host(st);
      const double tot = (double)std::accumulate(h.begin(), h.end(), 0ull);
      fprintf(stderr, "MM_SF_PROF share of cycles: zero+top %.3f | next head + resolve %.3f | scan %.3f | lists+count %.3f | window sums+alive+issue %.3f | phase 2 %.3f | survivors+end %.3f | total %.3g cycles over %d workgroups\n",
              h[0] / tot, (h[1] + h[7]) / tot, h[2] / tot, (h[3] + h[8]) / tot, (h[4] + h[9] + h[10] + h[11]) / tot, (h[5] + h[12]) / tot, h[6] / tot, tot, sf_grid);
      fprintf(stderr, "MM_SF_PROF in detail: top %.3f | first answers + second probes issued %.3f, their answers %.3f | scan %.3f | pieces loaded, counted, parked %.3f, next hashes asked for + barrier %.3f | "
                      "window sums %.3f, alive %.3f, barrier %.3f, hashes there + look-ups issued %.3f | bit tests + slots %.3f, barrier %.3f | survivors+end %.3f\n",
              h[0] / tot, h[7] / tot, h[1] / tot, h[2] / tot, h[8] / tot, h[3] / tot, h[9] / tot, h[10] / tot, h[4] / tot, h[11] / tot, h[12] / tot, h[5] / tot, h[6] / tot);
    }
  }

  int64_t hits_of(int64_t r) const { return (int64_t)(M->h_read_hit_off[(size_t)r + 1] - M->h_read_hit_off[(size_t)r]); }

  // ---- K4a: up to 4096 hits per read the LDS radix sort, beyond that the device's segmented radix sort (50 kb reads: 7.9 -> 7.0 ms against a sort per read)
  void sort_hits() {
    if (total_hits > 0) {
      const size_t t_sh = T.begin(&M->stats.ms_sort_hits);
      hl("K4 hits alloc + emit launch");
      int key_bits = 32; while (key_bits < 64 && ((int64_t)1 << (key_bits - 32)) < I->n_contigs) ++key_bits;
      if (sort_hits_radix(key_bits)) sort_hits_segmented(key_bits);
      T.end(t_sh);
    }
    hl("K4 launches + sync");
  }

  // the LDS radix sort over the reads of up to 4096 hits; true: longer lists are left
  bool sort_hits_radix(int key_bits) {
    static_assert(ipt_list_is<1, 2, 3, 4, 6, 8, 12, 16>(HIT_SORT_IPTS), "the dispatch below lists the classes of mm_size_classes.hpp");
    uint64_t left_seen = 0;
    const ReadBins RB = bin_reads(n, N_HIT_SORT_CLASSES, [&](int64_t r) -> int {
      const uint64_t c = (uint64_t)hits_of(r);
      left_seen |= (uint64_t)(c > HIT_SORT_LDS_MAX);
      return hit_sort_class_index(c);                          // (zero or one hit: nothing to sort; more than 4096: left)
    });
    hl("K4 bin");
    DBuf<int32_t> list(std::max<size_t>(RB.order.size(), 1));
    list.upload(RB.order.data(), RB.order.size(), st);
    hl("K4 list upload");
    size_t at = 0;
    for (auto& run : RB.runs) {
      const int32_t* lp = list.p + at;
      dispatch<1, 2, 3, 4, 6, 8, 12, 16>(HIT_SORT_IPTS[run.first], [&](auto tag) {
        constexpr int IPT = decltype(tag)::value;
        using SortT = rocprim::block_radix_sort<uint64_t, 256, IPT>;
        const size_t lds = sizeof(typename SortT::storage_type) + 16;
        if (lds > 48 * 1024) MM_HIP(hipFuncSetAttribute((const void*)sort_hits_radix_kernel<IPT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        sort_hits_radix_kernel<IPT><<<dim3((unsigned)run.second), dim3(256), lds, st>>>(M->hits.p, M->read_hit_off.p, lp, key_bits, sw.use_filter ? stage.p : nullptr, sw.use_filter ? stage_off.p : nullptr);
      });
      MM_KERNEL_CHECK();
      at += run.second;
    }
    MM_HIP(mm::stream_sync(st));                          // RB.order is the source of the async upload
    return left_seen != 0;
  }

  // Reads of more than 4096 hits (beyond ~30 kb): the device's segmented radix sort over exactly these reads' ranges.  When they are a
  // minority of the batch their ranges are gathered into a compact buffer first, so that the scratch is twice their hits instead of a
  // copy of all hits.  The sort counts its keys in 32 bits: a batch with max_keys hits or more goes through it as consecutive runs of
  // reads of fewer than max_keys hits each, every run through the compact buffer.
  void sort_hits_segmented(int key_bits) {
    const uint64_t max_keys = sw.segsort_max_keys;
    std::vector<int32_t> seg_reads;                               // ascending
    std::vector<uint64_t> hb, he, cb, ce;                         // per read: its range in hits[], and in the compact buffer of its run
    std::vector<size_t> run_at{0};                                // first read of every run (+ end)
    uint64_t in_run = 0, longest_run = 0;
    for (int64_t r = 0; r < n; ++r) {
      const uint64_t c = (uint64_t)hits_of(r);
      if (c <= HIT_SORT_LDS_MAX) continue;
      MM_REQUIRE(c < max_keys, MM_ERR_LIMIT, "one read has more seed hits than a segmented sort takes (2^32 - 1, or MM_SEGSORT_MAX_KEYS)");
      if (in_run + c >= max_keys) { run_at.push_back(seg_reads.size()); in_run = 0; }
      seg_reads.push_back((int32_t)r);
      hb.push_back(M->h_read_hit_off[(size_t)r]); he.push_back(M->h_read_hit_off[(size_t)r + 1]);
      cb.push_back(in_run); in_run += c; ce.push_back(in_run);
      longest_run = std::max(longest_run, in_run);
    }
    const size_t ns = seg_reads.size();
    run_at.push_back(ns);
    // one call over everything: in place where these reads are most of the batch
    const bool compact = run_at.size() > 2 || 2 * longest_run <= (uint64_t)total_hits || (uint64_t)total_hits >= max_keys;
    DBuf<uint64_t> d_hb(ns), d_he(ns), d_cb(ns), d_ce(ns);
    d_hb.upload(hb.data(), ns, st); d_he.upload(he.data(), ns, st);
    auto seg_sort = [&](uint64_t* in, uint64_t* out, uint64_t count, size_t nseg, uint64_t* begins, uint64_t* ends) {
      with_scratch([&](void* t, size_t& b) { return rocprim::segmented_radix_sort_keys(t, b, in, out, (unsigned int)count, (unsigned int)nseg, begins, ends, 0, key_bits, st); });
    };
    if (compact) {
      d_cb.upload(cb.data(), ns, st); d_ce.upload(ce.data(), ns, st);
      DBuf<uint64_t> packed((size_t)longest_run), sorted((size_t)longest_run);
      for (size_t k = 0; k + 1 < run_at.size(); ++k) {             // (on one stream: a run's buffers are free again when the next run gathers into them)
        const size_t i0 = run_at[k], nr = run_at[k + 1] - i0;
        move_ranges_kernel<<<dim3((unsigned)nr), dim3(256), 0, st>>>(M->hits.p, d_hb.p + i0, d_he.p + i0, packed.p, d_cb.p + i0);
        MM_KERNEL_CHECK();
        seg_sort(packed.p, sorted.p, ce[i0 + nr - 1], nr, d_cb.p + i0, d_ce.p + i0);
        move_ranges_kernel<<<dim3((unsigned)nr), dim3(256), 0, st>>>(sorted.p, d_cb.p + i0, d_ce.p + i0, M->hits.p, d_hb.p + i0);
        MM_KERNEL_CHECK();
      }
      MM_HIP(mm::stream_sync(st));
    } else {
      DBuf<uint64_t> sorted((size_t)total_hits);
      seg_sort(M->hits.p, sorted.p, (uint64_t)total_hits, ns, d_hb.p, d_he.p);
      move_ranges_kernel<<<dim3((unsigned)ns), dim3(256), 0, st>>>(sorted.p, d_hb.p, d_he.p, M->hits.p, d_hb.p);
      MM_KERNEL_CHECK();
      MM_HIP(mm::stream_sync(st));
    }
  }

  // ---- K4b: count, scan, write.  Leaves t_l1 open: it ends behind the write kernel (l2) or where there is nothing to write (no_candidates)
  void l1_candidates() {
    t_l1 = T.begin(&M->stats.ms_l1_scan);
    cand_n.alloc((size_t)n + 1); cand_n.zero(st);
    M->cand_off.alloc((size_t)n + 2);
    const unsigned rblk = (unsigned)ceil_div(std::max<int64_t>(n, 1), 128);
    if (n > 0) {
      if (sw.l1_serial) l1_scan_kernel<false><<<dim3(rblk), dim3(128), 0, st>>>(M->hits.p, M->read_hit_off.p, M->d_read_len.p, M->min_hits.p, n, cand_n.p, nullptr, nullptr, nullptr);
      else l1_wave_kernel<false><<<dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, st>>>(M->hits.p, M->read_hit_off.p, M->d_read_len.p, M->min_hits.p, n, cand_n.p, nullptr, nullptr, nullptr, nullptr);
      MM_KERNEL_CHECK();
    }
    exclusive_scan_u32_u64(cand_n.p, n, M->cand_off.p, scan_tmp, st);
    M->h_cand_off = M->cand_off.to_host(st, (size_t)n + 1);
    hl("L1 count + cand_off download");
    ncand = (int64_t)M->h_cand_off[(size_t)n];
    M->n_cand = ncand;
    M->stats.n_candidates = ncand;
    MM_REQUIRE(ncand < (1LL << 31), MM_ERR_LIMIT, "more than 2^31 L1 candidates in one batch");
    M->cand.alloc((size_t)std::max<int64_t>(3 * ncand, 1));
    M->cand_read.alloc((size_t)std::max<int64_t>(ncand, 1));
    M->l2.alloc((size_t)std::max<int64_t>(ncand, 1));
    cand_hint.alloc((size_t)std::max<int64_t>(ncand, 1));
    const bool no_hint = sw.l1_serial || sw.l2_no_fuse;
    if (no_hint) cand_hint.zero(st);                               // (0: no prediction, the masks of the band come from a second pass over the stream)
    M->rec_off.alloc((size_t)n + 1);
    if (ncand == 0) return;
    if (sw.l1_serial) l1_scan_kernel<true><<<dim3(rblk), dim3(128), 0, st>>>(M->hits.p, M->read_hit_off.p, M->d_read_len.p, M->min_hits.p, n, nullptr, M->cand_off.p, M->cand.p, M->cand_read.p);
    else l1_wave_kernel<true><<<dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, st>>>(M->hits.p, M->read_hit_off.p, M->d_read_len.p, M->min_hits.p, n, nullptr, M->cand_off.p, M->cand.p, M->cand_read.p, no_hint ? nullptr : cand_hint.p);
    MM_KERNEL_CHECK();
    T.end(t_l1);
  }

  // ---- K5/K6 launch helpers: the arguments every call site shares come from the run, the LDS size from the class
  // l2_kernel (mm_l2.hpp).  SKIP: hands reads shorter than w + k back through ovf and takes its scratch slot through slot_flags; the
  // literal full slide (!SKIP) does neither.  One wave per candidate of `list`.
  template <bool SKIP>
  void launch_l2(const int32_t* list, size_t nl, int sm, uint8_t* amb_ptr, uint8_t* masks, int n_slots) {
    const size_t lds = l2_lds_bytes(sm, SKIP);
    set_lds((const void*)l2_kernel<SKIP>, lds);
    l2_kernel<SKIP><<<dim3((unsigned)nl), dim3(64), lds, st>>>(IV, M->cand.p, M->cand_read.p, M->sk_hash.p, M->sk_strand.p,
        M->mz.off.p, M->sk_n.p, M->d_read_len.p, M->accept_min.p, P.k, P.w, sm, M->l2.p, counters.p, list, SKIP ? ovf.p : nullptr, SKIP ? ovf_n.p : nullptr, amb_ptr,
        masks, SKIP ? slot_flags_p() : nullptr, n_slots);
    MM_KERNEL_CHECK();
  }
  // l2z_kernel (mm_l2z.hpp), groups of up to NW candidates of a read
  template <int NW, int NWQ, bool QLDS>
  void launch_l2z(size_t grid, hipStream_t s, int sm, const int32_t* g0, const int32_t* gn, void* lists, uint8_t* masks, int n_slots) {
    const int bbl = l2z_bloom_log2(sm);
    const size_t lds = l2z_lds_bytes(sm, NWQ, QLDS, bbl, NW);
    set_lds((const void*)l2z_kernel<NW, NWQ, QLDS>, lds);
    l2z_kernel<NW, NWQ, QLDS><<<dim3((unsigned)grid), dim3(64 * NW), lds, s>>>(IV, M->cand.p, M->cand_read.p, M->sk_hash.p, M->sk_strand.p, M->mz.off.p, M->sk_n.p, M->d_read_len.p,
        M->accept_min.p, P.k, P.w, sm, bbl, M->l2.p, counters.p, g0, gn, ovf.p, ovf_n.p, sk->big.p, sk->big_n.p, amb_used_p, (uint32_t*)lists, masks, slot_flags_p(), n_slots, cand_hint.p, cand_rng.p);
    MM_KERNEL_CHECK();
  }
  // the wide form: class C, the zone kernels' big list, the redo of ambiguous votes, every class under MM_L2_V1
  void launch_l2_wide(const int32_t* list, size_t nl, int sm, uint8_t* amb_ptr) { launch_l2<true>(list, nl, sm, amb_ptr, masks_for(nl), (int)slots_of(nl)); }
  // the literal full slide over `list`
  void launch_l2_full(const int32_t* list, size_t nl, uint8_t* amb_ptr) { launch_l2<false>(list, nl, M->smax, amb_ptr, nullptr, 0); }

  // scratch slots of the skip kernels: twice as many as waves can be resident (the 10 kb class keeps 24 per CU, the long-read classes 8-12), so that a
  // wave finds a free one at its first or second try
  unsigned int* slot_flags_p() const { return sw.l2_no_slots ? nullptr : sk->slot_flags.p; }
  size_t max_slots(int nwq) const { return sw.l2_no_slots ? (size_t)1 << 40 : sw.l2_slots ? sw.l2_slots : (size_t)ctx->cus * (nwq == 2 ? 64 : 32); }
  size_t slots_of(size_t n_waves, int nwq = 8) const { return std::min((std::max<size_t>(n_waves, 1) + 7) / 8 * 8, max_slots(nwq)); }   // (a multiple of 8: one share per XCD)
  uint8_t* masks_for(size_t n_waves) { return (uint8_t*)ctx->l2_masks.at_least(ctx->alloc, slots_of(n_waves) * l2_skip_bytes(L2_NWQ)); }
  // the zone kernels' matched lists and masks: one slot range per wave of a launch (the launches of a batch share the buffers)
  void* lists_for(size_t n_waves, int nwq) { return ctx->l2_lists.at_least(ctx->alloc, slots_of(n_waves, nwq) * l2z_list_bytes(nwq)); }
  uint8_t* zmasks_for(size_t n_waves, int nwq) { return (uint8_t*)ctx->l2_masks.at_least(ctx->alloc, slots_of(n_waves, nwq) * l2z_mask_bytes(nwq)); }

  // ---- K5/K6
  void l2() {
    l2_setup();
    const size_t t_l2 = T.begin(&M->stats.ms_l2);
    l2_dense_beyond_limit();
    if (!sw.l2_skip) l2_full_slide(); else l2_skip_classes();
    l2_stats_kernel<<<dim3((unsigned)std::min<int64_t>(ceil_div(ncand, 256), 1024)), dim3(256), 0, st>>>(M->l2.p, ncand, counters.p);
    MM_KERNEL_CHECK();
    T.end(t_l2);
    hl("K5 wait");
    auto hc = counters.to_host(st);
    M->stats.sum_l2_stream_entries = (int64_t)hc[0];
    M->stats.sum_l2_evals = (int64_t)hc[1];
    M->stats.n_l2_rebuilds = (int64_t)hc[2];
    if (sw.l2_phases) { fprintf(stderr, "l2 rounds %llu zone passes %llu; ", hc[15], hc[12]); fprintf(stderr, "l2 phase clocks [setup passA bounds rebuild slide passB vote]:"); for (int i = 0; i < 7; ++i) fprintf(stderr, " %.3g", (double)hc[3 + i]); fprintf(stderr, "\n"); }
  }

  // ranges, the device's groups of the 10 kb class, the giant list, counters and debug word, the hand-back list; ends with the eager tie-break's strands in place
  void l2_setup() {
    if (!sw.l2_no_ranges) {
      cand_rng.alloc(2 * (size_t)ncand);
      l2_ranges_kernel<<<dim3((unsigned)ceil_div(ncand, 256)), dim3(256), 0, st>>>(IV, M->cand.p, M->cand_read.p, M->d_read_len.p, ncand, cand_rng.p);
      MM_KERNEL_CHECK();
    }
    grp_ctr.alloc(4);
    if (sw.dev_groups) {
      d_gA0.alloc((size_t)ncand); d_gAn.alloc((size_t)ncand); d_gS0.alloc((size_t)ncand); d_gSn.alloc((size_t)ncand);
      grp_ctr.zero(st);
      l2_group_kernel<<<dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st>>>(M->cand_off.p, M->sk_n.p, M->d_read_len.p, n, min_mapped_len(), sw.dense_from,
                                                                            sw.no_small_groups ? 1 : 0, d_gA0.p, d_gAn.p, d_gS0.p, d_gSn.p, grp_ctr.p);
      MM_KERNEL_CHECK();
    }
    const size_t lds_wide = l2_lds_bytes(M->smax, sw.l2_skip);
    // Sketches of >= 32768 hashes (L2_SKETCH_LIMIT): the rebuild's 1024-bucket histogram would be as coarse as the 64-rank pivot
    // zone, and the window state of the full slide no longer fits LDS either -> always the dense path, state in global memory.
    for (int64_t r = 0; r < n && M->stats.n_reads_giant > 0; ++r) {
      const int sr = M->h_sk_n[(size_t)r];
      if (sr < L2_SKETCH_LIMIT) continue;
      smG = std::max(smG, sr);
      for (uint64_t c0 = M->h_cand_off[(size_t)r]; c0 < M->h_cand_off[(size_t)r + 1]; ++c0) listG.push_back((int32_t)c0);
    }
    MM_REQUIRE(lds_wide <= 160 * 1024, MM_ERR_LIMIT, "L2 window state does not fit LDS");
    counters.alloc(16); counters.zero(st);
    if (sw.has_l2_debug_word()) {
      const unsigned long long v = sw.l2_debug_word();
      MM_HIP(hipMemcpyAsync(counters.p + 11, &v, sizeof v, hipMemcpyHostToDevice, st));
      MM_HIP(mm::stream_sync(st));
    }
    ovf.alloc((size_t)ncand);
    ovf_n.alloc(1); ovf_n.zero(st);
    if (!lazy_reads.empty()) { amb_used.alloc((size_t)n); amb_used.zero(st); }
    amb_used_p = lazy_reads.empty() ? nullptr : amb_used.p;
    finish_tiebreak();                                           // strands of ambiguous sketches: needed by the vote only
  }

  // Long reads: the window state in global memory, one wave per candidate (mm_l2_dense.hpp).  `list`: candidates, those of a read
  // consecutive; smax_l: largest sketch among them.
  void l2_dense(const std::vector<int32_t>& list, int smax_l, uint8_t* amb_ptr) {
    if (list.empty()) return;
    const size_t nl = list.size();
    DBuf<int32_t> d_list(nl); d_list.upload(list.data(), nl, st);
    DBuf<L2Range> d_rng(nl);
    l2_range_kernel<<<dim3((unsigned)ceil_div((int64_t)nl, 4)), dim3(256), 0, st>>>(IV, M->cand.p, M->cand_read.p, M->d_read_len.p, d_list.p, (int)nl, d_rng.p);
    MM_KERNEL_CHECK();
    std::vector<L2Range> rng = d_rng.to_host(st);               // (also keeps `list` alive until its upload is done)
    std::vector<uint64_t> coff(nl + 1, 0);
    for (size_t i = 0; i < nl; ++i) coff[i + 1] = coff[i] + (uint64_t)std::max(rng[i].m, 0);
    std::vector<int32_t> cr = M->cand_read.to_host(st, (size_t)ncand);
    std::vector<int32_t> gfirst;                               // one classification workgroup per read
    for (size_t i = 0; i < nl; ++i) if (i == 0 || cr[(size_t)list[i]] != cr[(size_t)list[i - 1]]) gfirst.push_back((int32_t)i);
    gfirst.push_back((int32_t)nl);
    DBuf<uint64_t> d_coff(nl + 1); d_coff.upload(coff.data(), nl + 1, st);
    DBuf<int32_t> d_gf(gfirst.size()); d_gf.upload(gfirst.data(), gfirst.size(), st);
    DBuf<uint32_t> codes((size_t)std::max<uint64_t>(coff[nl], 1));
    const int q_in_lds = smax_l <= LD_Q_LDS_MAX ? 1 : 0;
    const size_t lds = ((size_t)((LD_TSIZE + 3) & ~3) + (q_in_lds ? (size_t)smax_l + 4 : 0)) * 4;
    set_lds((const void*)l2_codes_kernel, lds);
    l2_codes_kernel<<<dim3((unsigned)(gfirst.size() - 1)), dim3(256), lds, st>>>(IV, M->cand_read.p, M->sk_hash.p, M->mz.off.p, M->sk_n.p, d_list.p, d_gf.p,
                                                                                d_rng.p, d_coff.p, codes.p, q_in_lds);
    MM_KERNEL_CHECK();
    const unsigned slots = (unsigned)std::min<size_t>(nl, (size_t)ctx->cus * 12);
    DBuf<uint32_t> scratch((size_t)slots * l2_dense_slot_words(smax_l));
    DBuf<unsigned int> next(1); next.zero(st);
    l2_dense_kernel<<<dim3(slots), dim3(64), 0, st>>>(IV, M->cand.p, M->cand_read.p, M->sk_strand.p, M->mz.off.p, M->sk_n.p, M->d_read_len.p, M->accept_min.p,
                                                    P.k, P.w, smax_l, M->l2.p, d_list.p, (int)nl, d_rng.p, d_coff.p, codes.p, scratch.p, next.p, amb_ptr, sw.force_amb_redo ? 1 : 0,
                                                    sw.dense_no_stop ? 0 : 1);
    MM_KERNEL_CHECK();
    MM_HIP(mm::stream_sync(st));                          // host vectors above are upload sources; the buffers die with this scope
  }

  // sketches of >= L2_SKETCH_LIMIT hashes
  void l2_dense_beyond_limit() { l2_dense(listG, smG, amb_used_p); }

  // MM_L2_FULL=1: every window of every candidate below the giant class
  void l2_full_slide() {
    std::vector<int32_t> listF;
    for (int64_t r = 0; r < n; ++r) if (M->h_sk_n[(size_t)r] < L2_SKETCH_LIMIT)
      for (uint64_t c0 = M->h_cand_off[(size_t)r]; c0 < M->h_cand_off[(size_t)r + 1]; ++c0) listF.push_back((int32_t)c0);
    DBuf<int32_t> d_listF(listF.size());
    if (!listF.empty()) {
      d_listF.upload(listF.data(), listF.size(), st);
      launch_l2_full(d_listF.p, listF.size(), amb_used_p);
    }
    MM_HIP(mm::stream_sync(st));                          // listF is the source of the async upload
  }

  // Reads are grouped by sketch size so that one long read does not size the LDS state (and the occupancy) of all:
  //   A  s <= 3072   (reads up to ~14 kb at w=8)  zone kernel: up to 4 candidates of a read per workgroup share the sketch,
  //                                                masks for 8 192 streamed entries (groups of one or two: two-wave workgroups)
  //   B  s <= 7168   (~32 kb)                      zone kernel with masks for 32 768 entries, the sketch left in global memory
  //   D  s <= 16384  (~74 kb)                      as B, launched separately so that B keeps its smaller LDS area
  //   C  larger                                    l2_kernel's wide form: one wave per workgroup and candidate, 32 768 entries
  // (MM_L2_V1: A, B and D join C; MM_L2_V1_LONG: B and D do.)
  // Reads shorter than w+k are handed back by these kernels and go through the literal full slide.
  void l2_skip_classes() {
    sk = std::make_unique<SkipClasses>();
    sk->slot_flags.alloc(std::max((size_t)ctx->cus * 64, sw.l2_slots)); sk->slot_flags.zero(st);   // (MM_L2_SLOTS may ask for more slots than cus * 64)
    sk->big.alloc((size_t)(sw.v2 ? ncand : 1));
    sk->big_n.alloc(1); sk->big_n.zero(st);
    l2_host_groups();
    l2_dense(sk->listL, sk->smL, amb_used_p);
    sk->d_gB0.alloc(sk->gB0.size()); sk->d_gBn.alloc(sk->gBn.size()); sk->d_listC.alloc(sk->listC.size());
    sk->nA = sk->gctr[0]; sk->nS = sk->gctr[1];
    if (!sw.dev_groups) {
      const size_t nA = sk->nA = sk->gA0.size(), nS = sk->nS = sk->gS0.size();
      d_gA0.alloc(std::max<size_t>(nA, 1)); d_gAn.alloc(std::max<size_t>(nA, 1)); d_gS0.alloc(std::max<size_t>(nS, 1)); d_gSn.alloc(std::max<size_t>(nS, 1));
      d_gA0.upload(sk->gA0.data(), nA, st); d_gAn.upload(sk->gAn.data(), nA, st); d_gS0.upload(sk->gS0.data(), nS, st); d_gSn.upload(sk->gSn.data(), nS, st);
    }
    sort_by_position(d_gA0, d_gAn, sk->nA);
    sort_by_position(d_gS0, d_gSn, sk->nS);
    l2_short_class();
    l2_long_class(sk->gB0, sk->gBn, sk->d_gB0, sk->d_gBn, sk->smB);
    sk->d_gD0.alloc(sk->gD0.size()); sk->d_gDn.alloc(sk->gDn.size());
    l2_long_class(sk->gD0, sk->gDn, sk->d_gD0, sk->d_gDn, sk->smD);
    if (!sk->listC.empty()) {
      sk->d_listC.upload(sk->listC.data(), sk->listC.size(), st);
      launch_l2_wide(sk->d_listC.p, sk->listC.size(), sk->smC, amb_used_p);
    }
    hl("K5 uploads + launches");
    // mm_map_batch_phased, stage 2: the last big kernel is enqueued.  (Here, before the wait below for the hand-back counters, so that the next step's
    // minimizer can fill the CUs the zone kernels leave as they drain; the rare big-list launch behind the wait is not waited for.)
    if (M->at_stage) M->at_stage(M->at_stage_user, 2);
    l2_handbacks();
    l2_redo_ambiguous();
    M->stats.n_l2_wide_redo = sk->n_redo + sk->n_fallback + sk->n_big;
    sk.reset();
  }

  // the host's classes: everything the device did not group
  void l2_host_groups() {
    SkipClasses& s = *sk;
    hl("K5 prep before grouping");
    if (sw.dev_groups) s.gctr = grp_ctr.to_host(st);               // (waits for the L1 kernel and the grouping kernel)
    s.smA = (int)s.gctr[3];
    for (int64_t r = 0; r < n && (!sw.dev_groups || s.gctr[2] > 0); ++r) {
      const uint64_t c_lo = M->h_cand_off[(size_t)r], c_hi = M->h_cand_off[(size_t)r + 1];
      if (c_lo == c_hi) continue;
      const int sr = M->h_sk_n[(size_t)r];
      if (sw.dev_groups && sr <= 3072 && !dense_read(r, sr)) continue;
      if (dense_read(r, sr)) {
        s.smL = std::max(s.smL, sr);
        for (uint64_t c0 = c_lo; c0 < c_hi; ++c0) s.listL.push_back((int32_t)c0);
        continue;
      }
      const bool zone = sr <= 3072 ? sw.v2 : sr <= 16384 && sw.v2_long;   // (else class C)
      if (zone && sr <= 7168) {
        auto& g0 = sr <= 3072 ? s.gA0 : s.gB0; auto& gn = sr <= 3072 ? s.gAn : s.gBn;
        (sr <= 3072 ? s.smA : s.smB) = std::max(sr <= 3072 ? s.smA : s.smB, sr);
        for (uint64_t c0 = c_lo; c0 < c_hi; c0 += 4) {
          const int32_t cnt = (int32_t)std::min<uint64_t>(4, c_hi - c0);
          // a workgroup holds the read's sketch once: four-wave workgroups with one or two candidates leave half of their waves'
          // LDS share idle (species of 1-12 strains: every candidate count occurs), those go to two-wave workgroups
          if (sr <= 3072 && cnt <= 2 && !sw.no_small_groups) { s.gS0.push_back((int32_t)c0); s.gSn.push_back(cnt); }
          else { g0.push_back((int32_t)c0); gn.push_back(cnt); }
        }
      } else if (zone) {
        s.smD = std::max(s.smD, sr);
        for (uint64_t c0 = c_lo; c0 < c_hi; c0 += 4) { s.gD0.push_back((int32_t)c0); s.gDn.push_back((int32_t)std::min<uint64_t>(4, c_hi - c0)); }
      } else if (sr < L2_SKETCH_LIMIT) {
        s.smC = std::max(s.smC, sr);
        for (uint64_t c0 = c_lo; c0 < c_hi; ++c0) s.listC.push_back((int32_t)c0);
      }                                                        // (larger: listG)
    }
    hl("K5 grouping");
  }

  // K5 workgroups in the order of where their first candidate lies (l2_group_keys_kernel)
  void sort_by_position(DBuf<int32_t>& g0, DBuf<int32_t>& gn, size_t ng) {
    if (!sw.sort_groups || ng < sw.group_sort_from || I->n_contigs <= 0) return;   // (small batches: three launches and a sort cost more than the order gives)
    DBuf<uint64_t> key(ng), val(ng), key2(ng), val2(ng);
    l2_group_keys_kernel<<<dim3((unsigned)ceil_div((int64_t)ng, 256)), dim3(256), 0, st>>>(g0.p, gn.p, M->cand.p, (int64_t)ng, key.p, val.p);
    int cbits = 1; while (cbits < 31 && ((int64_t)1 << cbits) < I->n_contigs) ++cbits;
    DBuf<uint8_t> tmp;
    sort_pairs(tmp, key.p, key2.p, val.p, val2.p, ng, 12, 32 + cbits, st);   // (positions at 4 kb granularity: bits 12 .. 32 + contig bits)
    l2_group_unpack_kernel<<<dim3((unsigned)ceil_div((int64_t)ng, 256)), dim3(256), 0, st>>>(val2.p, (int64_t)ng, g0.p, gn.p);
    MM_KERNEL_CHECK();
  }

  // The 10 kb class runs as two launches — groups of three or four candidates of a read in four-wave workgroups, groups of one or two in two-wave
  // workgroups — over disjoint candidates.  One behind the other on one stream each of them ends with a tail of a few long candidates on an otherwise
  // idle device (the two-wave launch keeps the VALU 55 % busy against 87 %; at an eighth of the batch the tails are a third of K5's time).  Side by
  // side — the second launch on the context's auxiliary stream, forked from and joined into the main one by events — each covers the other's tail.
  // Both take their scratch slots from ONE pool with ONE split by XCD (a slot's traffic stays in one L2, mm_l2.hpp), sized for the larger launch.
  // MM_L2_ONE_STREAM=1: one behind the other as until round 5 (cross-check and A/B).
  void l2_short_class() {
    const size_t nA = sk->nA, nS = sk->nS; const int smA = sk->smA;
    // side by side both launches draw on the pool at the same time: it holds a slot for every wave of both (as far as they can be resident — slots_of
    // caps it) so that small batches do not queue for each other's slots; one behind the other the larger launch sizes it
    const bool side_by_side = nA && nS && !sw.l2_no_slots && !sw.one_stream;   // (without slots the scratch is indexed by wave number of the launch: one launch at a time)
    const size_t n_waves = side_by_side ? nA * 4 + nS * 2 : std::max(nA * 4, nS * 2);
    void* const lists = !(nA || nS) ? nullptr : lists_for(n_waves, 2);
    uint8_t* const masks = !(nA || nS) ? nullptr : zmasks_for(n_waves, 2);
    const int n_slots = (int)slots_of(n_waves, 2);
    hipStream_t st_small = st;
    if (side_by_side) {
      ctx->aux_ready();
      st_small = ctx->aux_stream;
      MM_HIP(hipEventRecord(ctx->ev_fork, st));
      MM_HIP(hipStreamWaitEvent(st_small, ctx->ev_fork, 0));
    }
    if (nA) launch_l2z<4, 2, true>(nA, st, smA, d_gA0.p, d_gAn.p, lists, masks, n_slots);
    // groups of one or two candidates: a two-wave workgroup with the sketch in LDS holds 20 KB for two waves (16 waves per CU); with the sketch left
    // in global memory it holds 10 KB and the CU its 24 waves
    if (nS) launch_l2z<2, 2, false>(nS, st_small, smA, d_gS0.p, d_gSn.p, lists, masks, n_slots);
    if (side_by_side) {
      MM_HIP(hipEventRecord(ctx->ev_join, st_small));
      MM_HIP(hipStreamWaitEvent(st, ctx->ev_join, 0));
    }
  }

  // classes B and D: four-wave workgroups, masks for 32 768 entries
  void l2_long_class(const std::vector<int32_t>& g0, const std::vector<int32_t>& gn, DBuf<int32_t>& d_g0, DBuf<int32_t>& d_gn, int sm) {
    if (g0.empty()) return;
    const size_t ng = g0.size();
    d_g0.upload(g0.data(), ng, st); d_gn.upload(gn.data(), gn.size(), st);
    sort_by_position(d_g0, d_gn, ng);
    launch_l2z<4, 8, false>(ng, st, sm, d_g0.p, d_gn.p, lists_for(ng * 4, 8), zmasks_for(ng * 4, 8), (int)slots_of(ng * 4));
  }

  // candidates the skip kernels hand back (reads shorter than w+k): the literal full slide
  // read_ovf: ovf_n has not been read since the last launch that may add to it; otherwise h_ovf already holds it
  void l2_fallback(uint8_t* amb_ptr, bool read_ovf, unsigned int h_ovf) {
    if (read_ovf) {
      MM_HIP(hipMemcpyAsync(&h_ovf, ovf_n.p, sizeof h_ovf, hipMemcpyDeviceToHost, st));
      MM_HIP(mm::stream_sync(st));                      // also keeps the host lists alive until the uploads are done
    }
    if (!h_ovf) return;
    launch_l2_full(ovf.p, h_ovf, amb_ptr);
    ovf_n.zero(st);
    sk->n_fallback += h_ovf;
  }

  void l2_handbacks() {
    unsigned int h_ovf0 = 0;
    if (sw.v2) {                                                   // what the zone kernels handed back for its size: one wave per candidate, masks for 32 768 entries (beyond: every window)
      unsigned int h_big = 0;
      // both counters behind one wait: l2_kernel on the big list adds nothing to ovf_n (the zone kernels hand reads shorter than w + k to ovf before
      // they look at a candidate's size), so the fall-back below needs no second read of it
      MM_HIP(hipMemcpyAsync(&h_big, sk->big_n.p, sizeof h_big, hipMemcpyDeviceToHost, st));
      MM_HIP(hipMemcpyAsync(&h_ovf0, ovf_n.p, sizeof h_ovf0, hipMemcpyDeviceToHost, st));
      MM_HIP(mm::stream_sync(st));                        // also keeps the host lists alive until the uploads are done
      if (h_big) {
        launch_l2_wide(sk->big.p, h_big, std::max(std::max(sk->smA, sk->smB), sk->smD), amb_used_p);
        sk->n_big = h_big;
      }
    }
    l2_fallback(amb_used_p, !sw.v2, h_ovf0);
  }

  // votes that read an unresolved strand: resolve those reads, redo their candidates
  void l2_redo_ambiguous() {
    if (lazy_reads.empty()) return;
    std::vector<uint8_t> used = amb_used.to_host(st, (size_t)n);
    std::vector<int64_t> fix;
    for (int64_t r : lazy_reads) if (used[(size_t)r]) fix.push_back(r);
    if (fix.empty()) return;
    start_tiebreak(fix)();
    std::vector<int32_t> redo, redoL; int smR = 0, smRL = 0;   // redoL: reads of the dense path (long sketches) go through it again
    for (int64_t r : fix) {
      const int sr = M->h_sk_n[(size_t)r];
      const bool dense_r = sr >= L2_SKETCH_LIMIT || (sr >= sw.dense_from && M->read_len[(size_t)r] >= min_mapped_len());
      (dense_r ? smRL : smR) = std::max(dense_r ? smRL : smR, sr);
      for (uint64_t c0 = M->h_cand_off[(size_t)r]; c0 < M->h_cand_off[(size_t)r + 1]; ++c0) (dense_r ? redoL : redo).push_back((int32_t)c0);
    }
    l2_dense(redoL, smRL, nullptr);
    sk->n_redo += (int64_t)redoL.size();
    DBuf<int32_t> d_redo(std::max<size_t>(redo.size(), 1)); d_redo.upload(redo.data(), redo.size(), st);
    if (!redo.empty()) {
      launch_l2_wide(d_redo.p, redo.size(), smR, nullptr);
      l2_fallback(nullptr, true, 0);
    }
    MM_HIP(mm::stream_sync(st));
    sk->n_redo += (int64_t)redo.size();
  }

  // ---- compaction: accepted candidates -> records in read order
  void compact() {
    finish_tiebreak();
    const size_t t_cp = T.begin(&M->stats.ms_compact);
    DBuf<uint32_t> flag((size_t)ncand);
    DBuf<uint64_t> rank((size_t)ncand + 1);
    accept_flags_kernel<<<dim3((unsigned)ceil_div(ncand, 256)), dim3(256), 0, st>>>(M->l2.p, ncand, flag.p);
    MM_KERNEL_CHECK();
    exclusive_scan_u32_u64(flag.p, ncand, rank.p, scan_tmp, st);
    uint64_t nrec = 0;
    MM_HIP(hipMemcpyAsync(&nrec, rank.p + ncand, sizeof nrec, hipMemcpyDeviceToHost, st));
    MM_HIP(mm::stream_sync(st));
    M->n_rec = (int64_t)nrec;
    M->rec.alloc((size_t)std::max<uint64_t>(nrec, 1));
    write_records_kernel<<<dim3((unsigned)ceil_div(ncand, 256)), dim3(256), 0, st>>>(M->l2.p, M->cand_read.p, M->sk_n.p, flag.p, rank.p, ncand, M->rec.p);
    MM_KERNEL_CHECK();
    read_rec_bounds_kernel<<<dim3((unsigned)ceil_div(n + 1, 256)), dim3(256), 0, st>>>(M->cand_off.p, rank.p, n, M->rec_off.p);
    MM_KERNEL_CHECK();
    T.end(t_cp);
    MM_HIP(mm::stream_sync(st));
  }

  void no_candidates() {
    T.end(t_l1);
    finish_tiebreak();
    M->n_rec = 0;
    M->rec.alloc(1);
    M->rec_off.zero(st);
    MM_HIP(mm::stream_sync(st));
  }

  void finish() {
    M->h_rec_off = M->rec_off.to_host(st, (size_t)n + 1);
    T.end(t_total);
    T.collect();
    M->stats.n_mappings = M->n_rec;
    for (int64_t r = 0; r < n; ++r) if (M->h_rec_off[(size_t)r + 1] > M->h_rec_off[(size_t)r]) M->stats.n_reads_mapped++;
  }
};
}  // namespace

void map_batch(mm_ctx* ctx, const mm_index* I, const mm_seqset* reads, const mm_map_params& P, mm_mapping* M) {
  MapRun R(ctx, I, reads, P, M);
  R.begin();
  R.minimizers();
  R.sketch();
  if (!R.after_sketch()) return;
  R.tiebreak_lists();
  R.thresholds();
  R.seed_hits();
  R.sort_hits();
  R.l1_candidates();
  if (R.ncand > 0) { R.l2(); R.compact(); } else R.no_candidates();
  R.finish();
}

void probed_list_hist(mm_ctx* ctx, const mm_index* I, const mm_mapping* M, int nb, int64_t* hist) {
  hipStream_t st = ctx->stream;
  DBuf<unsigned long long> d((size_t)nb);
  d.zero(st);
  if (M->n_reads > 0)
    probed_list_hist_kernel<<<dim3((unsigned)M->n_reads), dim3(256), 0, st>>>(make_view(I), M->sk_hash.p, M->mz.off.p, M->sk_n.p, nb, d.p);
  MM_KERNEL_CHECK();
  auto h = d.to_host(st);
  for (int i = 0; i < nb; ++i) hist[i] = (int64_t)h[(size_t)i];
}

}  // namespace mm
