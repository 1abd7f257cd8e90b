// The EM of `classify` over the devices: the loop with its three ways of adding the ranks' sums (run_em_sharded), and the bootstrap's replicates dealt
// to the devices (run_bootstrap).  Everything in here calls the C ABI; the cut of the reads into shards is arithmetic and lives in mapping_lines.hpp.
#pragma once
#include "classify_tables.hpp"
#include "cli_device.hpp"
#include "cli_switches.hpp"
#include <climits>
#include <condition_variable>

namespace {

// The EM loop of classify across devices (meta::doEM, fEM.h:501-661).  The reads are sharded contiguously (em_shard), every rank computes the
// per-taxon posterior sums and the log-likelihood of its reads, the sums of the ranks are added (the merge of the per-thread sums, :583-600),
// and every rank normalises and evaluates the stop rule (:624-639) on identical values.
//   Rccl  one ncclAllReduce(f64, T+1) per iteration inside the device-resident loop (mm_em_run / mm_em_continue): the production path
//   Host  each rank's partial sums (mm_em_iterate) added on the host in rank order — what the all-reduce delivers —; several ranks
//         may then share one device, which is how everything AROUND the collective is tested on a one-GPU box (--em-host-reduce)
//   None  one rank, no communicator
enum class EmReduce { None, Rccl, Host };
struct ThreadBarrier {
  std::mutex m; std::condition_variable cv; const size_t n; size_t waiting = 0, gen = 0;
  explicit ThreadBarrier(size_t n_) : n(n_) {}
  void wait() { std::unique_lock<std::mutex> lk(m); const size_t g = gen; if (++waiting == n) { waiting = 0; ++gen; cv.notify_all(); } else cv.wait(lk, [&] { return gen != g; }); }
};
void print_em_round(long long it, double ll, double ll_prev) {  // the per-round lines of the reference's log (fEM.h:503, :602-603, :631-632)
  std::cout << "EM round " << it << std::endl << "\n\tLog likelihood: " << ll << std::endl;
  if (it > 0) std::cout << "\tImprovement: " << ll - ll_prev << "\n\tRelative   : " << ll / ll_prev << std::endl;
}
// f: start frequencies in, final frequencies out; post[mapping], best[read] (index into the whole mapping list) out; lca (may be null): every
// rank's reads assigned behind its posteriors, the ranks' direct counts added; rounds (may be null): the EM rounds that were run
void run_em_sharded(const std::vector<Dev>& devs, EmReduce reduce, const std::vector<int64_t>& off, const std::vector<int32_t>& taxon,
                    const std::vector<double>& mapq, const std::vector<double>& inv, size_t NT, std::vector<double>& f,
                    std::vector<double>& post, std::vector<int64_t>& best, LcaJob* lca, const CliSwitches& sw, long long* rounds = nullptr) {
  const size_t G = devs.size();
  if (reduce == EmReduce::None && G != 1) die("internal error: several EM ranks without a reduction");
  char comm_id[MM_COMM_ID_BYTES];
  if (reduce == EmReduce::Rccl && mm_comm_unique_id(comm_id) != MM_OK) die("RCCL: cannot create a communicator id");
  const std::vector<double> f0 = f;
  std::vector<std::vector<double>> part(G, std::vector<double>(NT + 1, 0.0));   // Host: the ranks' partial sums of one iteration
  std::vector<double> f_cur = f0; bool host_stop = false; double ll_prev = 0;
  ThreadBarrier bar(G);
  const long long MAX_ITER = sw.em_max_iter;
  const int SLICE = sw.em_slice;
  on_each(G, [&](size_t d) {
    mm_ctx* ctx = devs[d].ctx;
    if (reduce == EmReduce::Rccl) ck(ctx, mm_comm_init(ctx, comm_id, (int)d, (int)G), "RCCL communicator");
    const EmShard sh = em_shard(off, G, d);
    const size_t n = sh.hi - sh.lo;
    mm_em* em; ck(ctx, mm_em_create(ctx, (int64_t)n, sh.soff.data(), taxon.data() + sh.e0, mapq.data() + sh.e0, inv.data() + sh.e0, (int32_t)NT, &em), "em");
    std::vector<double> fl(NT);
    if (reduce != EmReduce::Host) {
      // the loop itself runs on the device (E step, sums, all-reduce, normalisation and the stop rule per iteration, no host round
      // trip), in slices of <= 1024 iterations so that every round's log-likelihood reaches the log as in the reference
      std::vector<double> lls((size_t)std::min(SLICE, 1024));
      long long done = 0; double prev = 0;
      for (bool first = true;; first = false) {
        int n_iter = 0, stopped = 0;
        const int want = (int)std::min<long long>((long long)lls.size(), MAX_ITER - done);
        if (want <= 0) break;
        if (first) { ck(ctx, mm_em_run(em, f0.data(), want, fl.data(), lls.data(), (int)lls.size(), &n_iter), "em"); stopped = n_iter < want; }
        else ck(ctx, mm_em_continue(em, want, fl.data(), lls.data(), (int)lls.size(), &n_iter, &stopped), "em");
        if (d == 0) for (int it = 0; it < n_iter; ++it) { print_em_round(done + it, lls[(size_t)it], prev); prev = lls[(size_t)it]; }
        done += n_iter;
        if (stopped || n_iter == 0) break;
      }
      if (d == 0 && rounds) *rounds = done;
    } else {
      for (long long it = 0; it < MAX_ITER; ++it) {
        ck(ctx, mm_em_iterate(em, f_cur.data(), part[d].data(), &part[d][NT]), "em");
        bar.wait();
        if (d == 0) {                                            // the sum over the ranks, in rank order; normalisation (fEM.h:606-615); stop rule (:624-639)
          std::vector<double> tot(NT + 1, 0.0);
          for (size_t g = 0; g < G; ++g) for (size_t t = 0; t <= NT; ++t) tot[t] += part[g][t];
          double sum = 0; for (size_t t = 0; t < NT; ++t) sum += tot[t];
          for (size_t t = 0; t < NT; ++t) f_cur[t] = tot[t] / sum;
          const double ll = tot[NT];
          print_em_round(it, ll, ll_prev);
          if (rounds) *rounds = it + 1;
          if (it > 0 && (ll - ll_prev) <= 1 && (1 - ll / ll_prev) < 0.0001) host_stop = true;
          ll_prev = ll;
        }
        bar.wait();
        if (host_stop) break;
      }
      fl = f_cur;
    }
    std::vector<int64_t> bl(n);
    ck(ctx, mm_em_posteriors(em, fl.data(), post.data() + sh.e0, bl.data()), "posteriors");
    for (size_t i = 0; i < n; ++i) best[sh.lo + i] = bl[i] < 0 ? -1 : bl[i] + (int64_t)sh.e0;   // rank-local index -> index into the whole mapping list
    if (lca) {
      std::vector<int64_t> dl(lca->id.size());
      ck(ctx, mm_em_lca(em, fl.data(), (int32_t)lca->id.size(), lca->parent.data(), lca->taxon_node.data(), lca->tau, lca->node.data() + sh.lo, lca->mass.data() + sh.lo, dl.data()), "lca");
      std::lock_guard<std::mutex> lk(lca->m);
      for (size_t v = 0; v < dl.size(); ++v) lca->direct[v] += dl[v];
    }
    mm_em_destroy(em);
    bar.wait();                                                  // (every rank has read f_cur)
    if (d == 0) f = fl;
  });
}

// --bootstrap B: replicates 0..B-1 of the weighted EM (mm_em_bootstrap), started from the point estimate f, dealt to the devices in contiguous
// ranges; every device holds the whole EM problem and tiles its range to its free memory.  The result depends on neither.  A replicate that
// drew no read (e^-n of them for n mapped reads: small samples only) has no estimate and is left out of every statistic.
struct BootReplicates {
  std::vector<int32_t> pres; std::vector<double> f;              // the taxa with a mapping; the replicates' frequencies of those, [replicate][pres]
  std::vector<char> empty;                                       // [replicate]: it drew no read (mm_em_bootstrap: n_iter == 0) and has no estimate
};
BootReplicates run_bootstrap(const std::vector<Dev>& devs, const BootOpts& boot, const MappingLines& M, const ClassifyTables& C, const std::vector<double>& f) {
  BootReplicates R;
  const auto t0 = std::chrono::steady_clock::now();
  const size_t NT = C.taxa.size(), G = devs.size(), B = (size_t)boot.B;
  { std::vector<char> has(NT, 0); for (int32_t t : C.taxon) has[(size_t)t] = 1; for (size_t t = 0; t < NT; ++t) if (has[t]) R.pres.push_back((int32_t)t); }
  const size_t NP = R.pres.size();
  R.f.assign(B * NP, 0.0);
  R.empty.assign(B, 0);
  const int MAX_ITER = 10000;
  std::atomic<long long> at_cap{0}; std::atomic<int> it_min{INT_MAX}, it_max{0};
  on_each(G, [&](size_t d) {
    const size_t lo = B * d / G, hi = B * (d + 1) / G;
    if (hi <= lo) return;
    mm_ctx* ctx = devs[d].ctx;
    mm_em* em; ck(ctx, mm_em_create(ctx, (int64_t)M.NRD, M.off.data(), C.taxon.data(), C.mapq.data(), C.inv.data(), (int32_t)NT, &em), "bootstrap");
    uint64_t tot = 0, fr = 0;
    ck(ctx, mm_ctx_device_info(ctx, nullptr, 0, nullptr, &tot, &fr), "device info");
    // per replicate on the device: posteriors (8 B per mapping), frequencies and sums (8 B per taxon, ~3x), a little per read block; half of
    // the free memory (the logical devices of one GPU share it); on the host the call's f_out (8 B per taxon) within 1 GiB
    const double per_rep = 8.0 * ((double)C.taxon.size() + 3.0 * (double)NT + (double)M.NRD / 64.0) + 1024.0;
    const size_t by_dev = (size_t)std::max(1.0, (double)fr / (2.0 * G) / per_rep), by_host = std::max<size_t>(1, ((size_t)1 << 30) / (8 * std::max<size_t>(NT, 1)));
    const size_t tile = std::max<size_t>(1, std::min({hi - lo, by_dev, by_host}));
    std::vector<double> fo(tile * NT), llo(tile); std::vector<int32_t> nit(tile), stp(tile);
    for (size_t r0 = lo; r0 < hi; r0 += tile) {
      const size_t n = std::min(tile, hi - r0);
      ck(ctx, mm_em_bootstrap(em, f.data(), (int32_t)r0, (int32_t)n, boot.seed, nullptr, MAX_ITER, fo.data(), llo.data(), nit.data(), stp.data()), "bootstrap");
      for (size_t k = 0; k < n; ++k) {
        for (size_t j = 0; j < NP; ++j) R.f[(r0 + k) * NP + j] = fo[k * NT + (size_t)R.pres[j]];
        if (nit[k] == 0) { R.empty[r0 + k] = 1; continue; }
        if (!stp[k]) ++at_cap;
        int v = it_min.load(); while (nit[k] < v && !it_min.compare_exchange_weak(v, nit[k])) {}
        v = it_max.load(); while (nit[k] > v && !it_max.compare_exchange_weak(v, nit[k])) {}
      }
    }
    mm_em_destroy(em);
  });
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  const size_t n_empty = (size_t)std::count(R.empty.begin(), R.empty.end(), (char)1);
  const std::string left_out = std::to_string(n_empty) + " of " + std::to_string(B) + " drew no read and are left out";
  if (B - n_empty < 2) die("--bootstrap: " + left_out + ": fewer than two replicates to describe");
  std::cout << "Bootstrap: " << B << " replicates, seed " << boot.seed << ", " << it_min.load() << "-" << it_max.load() << " EM iterations per replicate, "
            << secs << " s on " << G << " device(s)" << (n_empty ? ", " + left_out : std::string()) << std::endl;
  if (at_cap) std::cerr << "Warning: " << at_cap.load() << " of " << B << " bootstrap replicates reached " << MAX_ITER << " EM iterations without meeting the stop rule." << std::endl;
  return R;
}

}  // namespace
