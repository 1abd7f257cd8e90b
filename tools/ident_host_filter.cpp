// The identity filter on ONE host thread through mm_ident_core.hpp (ident_filter_host), for tools/ident_filter_stats.py: the comparison figure beside
// the device's stage times.  Reads the raw little-endian arrays that the script left in DIR, prints its wall time and checksums of its results.
//   g++ -O2 -std=c++17 -o ident_host_filter tools/ident_host_filter.cpp && ident_host_filter DIR n_taxa thr
#include "../metamaps_amd/csrc/mm_ident_core.hpp"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>

template <class T> static std::vector<T> load(const std::string& fn) {
  FILE* f = fopen(fn.c_str(), "rb"); if (!f) { fprintf(stderr, "cannot open %s\n", fn.c_str()); exit(2); }
  fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
  std::vector<T> v((size_t)n / sizeof(T));
  if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const std::string d = std::string(argv[1]) + "/";
  const int64_t n_taxa = atoll(argv[2]); const double thr = atof(argv[3]);
  const auto off = load<int64_t>(d + "off"), best = load<int64_t>(d + "best");
  const auto taxon = load<int32_t>(d + "taxon");
  const auto ident = load<double>(d + "ident");
  const int64_t nr = (int64_t)off.size() - 1;
  if (mm::ident_args_check(nr, off.data(), taxon.data(), ident.data(), best.data(), n_taxa, thr)) return 3;
  const auto t0 = std::chrono::steady_clock::now();
  mm::IdentHostOut o;
  mm::ident_filter_host(nr, off.data(), taxon.data(), ident.data(), best.data(), n_taxa, thr, &o);
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  long long removed = 0; for (uint8_t x : o.taxon_removed) removed += x;
  printf("host filter, one thread: %.1f ms; %lld of the genomes removed, %zu reads and %zu entries kept, n_le %lld\n", 1e3 * secs, removed, o.read_src.size(), o.entry_src.size(),
         (long long)o.n_le);
  return 0;
}
