// The formatter of the mapping lines: the records of one batch -> the text of PREFIX, and what --then-classify keeps of every line.
#pragma once
#include "../cpu_budget.hpp"
#include "../task_pool.hpp"
#include "mapping_lines.hpp"
#include "cli_switches.hpp"
#include "fast_format.hpp"
#include <cmath>

namespace {

// records of one batch -> the text of PREFIX (computeMap.hpp:565-581 + the two fields of mapWrap.h:311-320), reads in order
// fields 10 and 13 of a mapping line are functions of (conserved sketches, sketch size) alone: formatted once per pair and kept.  The table belongs
// to the CALLER (one per formatting slot of a worker thread) and lives as long as that thread: the pool threads of format_records are new with every
// batch, and a table that was theirs (thread_local) was rebuilt — 0.8 MB cleared, every pair formatted again — by every one of them for every batch:
// 19 ms per batch of 85 000 lines, the whole of a worker's "finish" time.
struct FormatCache {
  struct Pair {
    uint64_t key;
    char ids[16], corr[16];
    uint8_t n_ids, n_corr;
    double ident;                                                  // the printed identity read back / 100 (what classify parses, fEM.h:264)
  };
  static constexpr size_t CB = 1 << 14;
  std::vector<Pair> slots; int k = -1;
  void prepare(int k_now) { if (slots.size() != CB || k != k_now) { slots.assign(CB, Pair{~0ull, {0}, {0}, 0, 0, 0.0}); k = k_now; } }
};
static void format_range(const std::vector<std::string>& names, const std::vector<int>& lens, const std::vector<int64_t>& off,
                         const std::vector<mm_map_record>& rec, const std::vector<std::string>& cname, const std::vector<int>& clen, int k,
                         size_t r0, size_t r1, std::string& out, FormatCache& fc, std::vector<LineMeta>* meta,
                         const int64_t* raw_end /* --hpc: field 9 of every record; else nullptr */) {
  out.clear();
  if (meta) { meta->clear(); meta->reserve((size_t)(off[r1] - off[r0])); }
  out.reserve((size_t)(off[r1] - off[r0]) * 160);
  // no printf anywhere on the line (fast_format.hpp) — 4.2 M lines took 2 s of the mapping phase of a million reads
  using Pair = FormatCache::Pair;
  fc.prepare(k);
  std::vector<Pair>& cache = fc.slots;
  std::string tmp;
  for (size_t r = r0; r < r1; ++r) {
    const int len = lens[r];
    for (int64_t i = off[r]; i < off[r + 1]; ++i) {
      const mm_map_record& x = rec[(size_t)i];
      const uint64_t key = (uint64_t)(uint32_t)x.sketch << 32 | (uint32_t)x.shared;
      Pair& P = cache[(size_t)((key * 0x9E3779B97F4A7C15ull) >> 50)];
      if (P.key != key) {
        float id; mm_identity(x.shared, x.sketch, k, &id, nullptr);
        tmp.clear(); append_g6(tmp, (double)id);                   // operator<<(float): %g with 6 significant digits; printed, then re-parsed (mapWrap.h:237)
        P.n_ids = (uint8_t)tmp.size(); memcpy(P.ids, tmp.data(), tmp.size());
        const double reported = strtod(tmp.c_str(), nullptr) / 100.0;
        P.ident = reported;
        const float corrected = std::exp(-(1 - reported));        // mapWrap.h:311
        tmp.clear(); append_g6(tmp, (double)(corrected * 100));
        P.n_corr = (uint8_t)tmp.size(); memcpy(P.corr, tmp.data(), tmp.size());
        P.key = key;
      }
      const long long stop = raw_end ? (long long)raw_end[(size_t)i] : (long long)x.ref_start + len - 1;   // field 9
      const size_t line_beg = out.size();
      out += names[r];
      out += ' '; append_int(out, len); out += " 0 "; append_int(out, len - 1); out += ' '; out += x.strand == 1 ? '+' : '-'; out += ' ';
      out += cname[(size_t)x.ref_contig];
      out += ' '; append_int(out, clen[(size_t)x.ref_contig]);
      out += ' '; append_int(out, x.ref_start); out += ' '; append_int(out, stop);
      out += ' '; out.append(P.ids, P.n_ids);
      out += ' '; append_int(out, x.shared); out += ' '; append_int(out, x.sketch);
      out += ' '; out.append(P.corr, P.n_corr);
      const size_t ls = out.size();
      out += ' '; append_g6(out, x.mapq);                          // :318-320
      if (meta) meta->push_back(LineMeta{(uint32_t)line_beg, (uint32_t)(ls - line_beg), (uint32_t)(out.size() - line_beg), (int32_t)x.ref_contig, (int32_t)len,
                                         (int32_t)x.ref_start, (int32_t)stop, P.ident, mapq_as_classify_reads_it(out.data() + ls + 1, out.size() - ls - 1)});
      out += '\n';
    }
  }
}
// the mapping lines of a batch (mapWrap.h:300-323): ranges of reads formatted by a few threads, joined in read order
void format_records(const std::vector<std::string>& names, const std::vector<int>& lens, const std::vector<int64_t>& off,
                    const std::vector<mm_map_record>& rec, const std::vector<std::string>& cname, const std::vector<int>& clen, int k, std::string& out,
                    std::vector<LineMeta>* meta, const int64_t* raw_end, const CliSwitches& sw) {
  const size_t n = names.size();
  const size_t per_part = sw.format_part;
  // (a quarter of the CPU budget per worker: four workers rarely format at the same moment)
  const size_t by_budget = (size_t)std::max(per_part < 10000 ? 8u : 1u, mm::cpu_budget() / 4);
  const size_t T = std::max<size_t>(1, std::min<size_t>({(size_t)8, by_budget, rec.size() / per_part + 1}));
  static thread_local std::vector<FormatCache> caches(8);          // (the calling thread's: a worker of mapDirectly formats batch after batch)
  if (T == 1) { format_range(names, lens, off, rec, cname, clen, k, 0, n, out, caches[0], meta, raw_end); return; }
  std::vector<size_t> cut(T + 1, n);
  cut[0] = 0;
  { size_t t = 1; for (size_t r = 0; r < n && t < T; ++r) if ((uint64_t)off[r] >= (uint64_t)rec.size() * t / T) cut[t++] = r; }
  static thread_local std::vector<std::string> part_store(8);      // (kept with their capacity: fresh text buffers are page faults, batch after batch)
  std::vector<std::string>& part = part_store;
  FormatCache* const fcs = caches.data();
  static thread_local std::vector<std::vector<LineMeta>> meta_store(8);
  std::vector<std::vector<LineMeta>>& metas = meta_store;        // (the CALLING thread's: the helpers below must not name the thread_local themselves)
  const auto q0 = std::chrono::steady_clock::now();
  std::vector<double> took(T, 0.0);
  auto timed = [&](size_t t) {
    const auto a = std::chrono::steady_clock::now();
    format_range(names, lens, off, rec, cname, clen, k, cut[t], cut[t + 1], part[t], fcs[t], meta ? &metas[t] : nullptr, raw_end);
    took[t] = std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count();
  };
  static thread_local TaskPool helpers(7);                         // (task_pool.hpp: the calling worker's own helpers, there from batch to batch)
  const auto q1 = q0;
  helpers.run(T, timed);
  const auto q2 = std::chrono::steady_clock::now();
  size_t total = 0; for (size_t t = 0; t < T; ++t) total += part[t].size();
  out.clear(); out.reserve(total);
  if (meta) { meta->clear(); meta->reserve(rec.size()); }
  for (size_t t = 0; t < T; ++t) {
    if (meta) for (LineMeta lm : metas[t]) { lm.beg += (uint32_t)out.size(); meta->push_back(lm); }
    out += part[t];
  }
  if (sw.format_trace) {
    const auto q3 = std::chrono::steady_clock::now();
    double mx = 0; for (double x : took) mx = std::max(mx, x);
    fprintf(stderr, "FORMAT_TRACE %zu records, %zu threads: all parts %.2f ms (own part %.2f ms, slowest part %.2f ms), join text %.2f ms\n", rec.size(), T,
            std::chrono::duration<double, std::milli>(q2 - q1).count(), took[0] * 1e3, mx * 1e3, std::chrono::duration<double, std::milli>(q3 - q2).count());
  }
}

}  // namespace
