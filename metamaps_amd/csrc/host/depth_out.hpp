// mapDirectly --depth [--depth-window W] [--depth-thresholds T1,T2,...] (implies --edit-distance; not in the reference): PREFIX.depth.bedgraph, .depth.windows
// and .depth.contigs, how evenly the PRIMARY alignments of the run are spread over every contig they touch (the definition: csrc/mm_depth_core.hpp; one
// mm_depth_profile call per query file on the first device, over the intervals --pileup keeps).  All three are plain text whatever --compress-output says; an
// empty run writes the first two empty and the header of the third alone.
//   PREFIX.depth.bedgraph  contigID  start  end  depth: the maximal runs of equal depth >= 1 (0-based, end exclusive), in the reference's order; no track line
//   PREFIX.depth.windows   contigID  start  end  sumDepth  covered  meanDepth: every window of W (default 1000, the window of .EM.contigCoverage) of every
//                          contig with a primary alignment; meanDepth is %.3f of sumDepth / (end - start)
//   PREFIX.depth.contigs   a # header, then per such contig: contigID length alignments covered sumDepth meanDepth medianDepth maxDepth breadth expectedBreadth
//                          ge<T1> ...; meanDepth %.3f; breadth = covered / length and expectedBreadth = 1 - exp(-sumDepth / length), what a uniform spread
//                          of that depth would cover, both %.6f; ge<T> the positions of depth >= T (default 1,5,10,30)
// Text, arrays and the option values only: nothing here calls the device.
#pragma once
#include "../mm_depth_core.hpp"
#include "pileup_out.hpp"
#include <cmath>
#include <cstdio>

namespace {

// the window and the thresholds: validated before any work; refused without --depth
struct DepthOpts { bool on = false; long long window = 1000; int n_thresholds = 4; int64_t thresholds[mmdp::MAX_THRESHOLDS] = {1, 5, 10, 30}; };
DepthOpts depth_options(const Options& o) {
  DepthOpts p;
  p.on = o.v.count("depth") != 0;
  auto integer_of = [](const std::string& v) -> long long {       // 1 to 999999999999, or -1
    const IntegerValue x = integer_value(v, 12);
    return x.ok ? (long long)x.value : -1;
  };
  if (o.v.count("depth-window")) {
    const std::string& v = o.v.at("depth-window");
    if (!p.on) die("--depth-window needs --depth");
    if (integer_of(v) < 1) die("--depth: --depth-window takes an integer from 1 to 999999999999, not '" + v + "'");
    p.window = integer_of(v);
  }
  if (o.v.count("depth-thresholds")) {
    const std::string& v = o.v.at("depth-thresholds");
    if (!p.on) die("--depth-thresholds needs --depth");
    const std::string what = "--depth: --depth-thresholds takes 1 to 8 ascending integers from 1 on, separated by commas, not '" + v + "'";
    p.n_thresholds = 0;
    for (size_t at = 0; at <= v.size();) {
      const size_t comma = std::min(v.find(',', at), v.size());
      const long long t = integer_of(v.substr(at, comma - at));
      if (t < 1 || p.n_thresholds == mmdp::MAX_THRESHOLDS || (p.n_thresholds > 0 && t <= p.thresholds[p.n_thresholds - 1])) die(what);
      p.thresholds[p.n_thresholds++] = t;
      at = comma + 1;
    }
  }
  return p;
}

// the runs in order: contigID start end depth
std::string depth_bedgraph_text(const std::vector<int32_t>& contig, const std::vector<int64_t>& start, const std::vector<int64_t>& end, const std::vector<uint32_t>& depth,
                                const std::vector<std::string>& cname) {
  std::string t;
  t.reserve(contig.size() * 40);
  for (size_t r = 0; r < contig.size(); ++r) {
    t += cname[(size_t)contig[r]]; t += '\t'; append_int(t, (long long)start[r]); t += '\t'; append_int(t, (long long)end[r]); t += '\t'; append_int(t, (long long)depth[r]); t += '\n';
  }
  return t;
}
void depth_append_fixed(std::string& t, double x, int digits) {
  char buf[64];
  t.append(buf, (size_t)snprintf(buf, sizeof buf, "%.*f", digits, x));
}
// the windows [win_off[j], win_off[j + 1]) of the listed contig[j]
std::string depth_windows_text(const std::vector<int32_t>& contig, const std::vector<int64_t>& win_off, const std::vector<int64_t>& sum, const std::vector<int64_t>& covered, long long window,
                               const std::vector<std::string>& cname, const std::vector<int>& clen) {
  std::string t;
  t.reserve(sum.size() * 56);
  for (size_t j = 0; j < contig.size(); ++j)
    for (int64_t k = win_off[j]; k < win_off[j + 1]; ++k) {
      int64_t a, b;
      mmdp::window_span(clen[(size_t)contig[j]], window, k - win_off[j], &a, &b);
      t += cname[(size_t)contig[j]]; t += '\t'; append_int(t, (long long)a); t += '\t'; append_int(t, (long long)b); t += '\t'; append_int(t, (long long)sum[(size_t)k]); t += '\t';
      append_int(t, (long long)covered[(size_t)k]); t += '\t'; depth_append_fixed(t, (double)sum[(size_t)k] / (double)(b - a), 3); t += '\n';
    }
  return t;
}
std::string depth_contigs_header(const DepthOpts& p) {
  std::string t = "#contigID\tlength\talignments\tcovered\tsumDepth\tmeanDepth\tmedianDepth\tmaxDepth\tbreadth\texpectedBreadth";
  for (int k = 0; k < p.n_thresholds; ++k) { t += "\tge"; append_int(t, (long long)p.thresholds[k]); }
  return t + "\n";
}
// stats: mmdp::STATS + n_thresholds counters per listed contig
std::string depth_contigs_text(const DepthOpts& p, const std::vector<int32_t>& contig, const std::vector<int64_t>& stats, const std::vector<std::string>& cname, const std::vector<int>& clen) {
  std::string t = depth_contigs_header(p);
  const size_t per = (size_t)(mmdp::STATS + p.n_thresholds);
  for (size_t j = 0; j < contig.size(); ++j) {
    const int64_t* s = &stats[j * per];
    const double len = (double)clen[(size_t)contig[j]];
    t += cname[(size_t)contig[j]]; t += '\t'; append_int(t, clen[(size_t)contig[j]]);
    for (int k : {mmdp::ALIGNMENTS, mmdp::COVERED, mmdp::SUM_DEPTH}) { t += '\t'; append_int(t, (long long)s[k]); }
    t += '\t'; depth_append_fixed(t, (double)s[mmdp::SUM_DEPTH] / len, 3);
    for (int k : {mmdp::MEDIAN_DEPTH, mmdp::MAX_DEPTH}) { t += '\t'; append_int(t, (long long)s[k]); }
    t += '\t'; depth_append_fixed(t, (double)s[mmdp::COVERED] / len, 6);
    t += '\t'; depth_append_fixed(t, 1.0 - std::exp(-(double)s[mmdp::SUM_DEPTH] / len), 6);
    for (int k = 0; k < p.n_thresholds; ++k) { t += '\t'; append_int(t, (long long)s[mmdp::STATS + k]); }
    t += '\n';
  }
  return t;
}

}  // namespace
