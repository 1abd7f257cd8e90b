// The host side of tools/edit_kernel_stats.py: csrc/mm_edit_core.hpp's edit_infix_host (two-pass wavefront alignment, one thread) over a sample of the
// jobs the device aligned.  Input lines: strand max_dist dist begin end =READ =WINDOW (dist begin end: what the device returned, window coordinates,
// -1 -1 -1 not aligned).  Prints the time, the jobs per second and how many answers differ from the device's.
#include "../metamaps_amd/csrc/mm_edit_core.hpp"
#include <chrono>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

int main() {
  struct Job { int strand; long long md, d, a, b; std::string q, w; };
  std::vector<Job> jobs;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    Job j;
    if (in >> j.strand >> j.md >> j.d >> j.a >> j.b >> j.q >> j.w) jobs.push_back(j);
  }
  size_t differ = 0; long long bases = 0;
  const auto t0 = std::chrono::steady_clock::now();
  for (const Job& j : jobs) {
    const mm::EditHostResult r = mm::edit_infix_host(j.q.data() + 1, (int64_t)j.q.size() - 1, j.strand, j.w.data() + 1, (int64_t)j.w.size() - 1, (int32_t)j.md);
    const bool same = r.dist < 0 ? j.d < 0 : (r.dist == j.d && r.begin == j.a && r.end == j.b);
    differ += !same; bases += (long long)j.q.size() - 1;
  }
  const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  printf("edit_infix_host, one thread: %zu jobs (%lld read bases) in %.1f ms, %.0f jobs/s; %zu answers differ from the device's\n", jobs.size(), bases, 1e3 * s,
         jobs.empty() ? 0.0 : (double)jobs.size() / s, differ);
  return differ ? 1 : 0;
}
