// Host harness of metamaps_amd/csrc/mm_ident_core.hpp for tests/test_ident_core.py (g++, plain and with the address / undefined-behaviour sanitizers).
// Reads whitespace-separated records from stdin:
//   F nr ne nt thr_bits  read_off[nr+1]  taxon[ne]  ident_bits[ne]  best[nr]
// and answers one line each: "refused CODE" where ident_args_check refuses, else the results of ident_filter_host as lists separated by ';':
//   sorted_max bits ; n_le ; taxon_reads ; taxon_median bits ; taxon_removed ; read_removed ; read_src ; entry_src ; read_off_out
#include "../metamaps_amd/csrc/mm_ident_core.hpp"
#include <cstdio>
#include <iostream>
#include <string>

template <class T> static std::vector<T> take(size_t n) { std::vector<T> v(n); for (auto& x : v) { long long y; std::cin >> y; x = (T)y; } return v; }
static std::vector<double> take_bits(size_t n) { std::vector<double> v(n); for (auto& x : v) { unsigned long long b; std::cin >> b; x = mm::ident_from_bits(b); } return v; }
template <class V> static void put(const V& v) { for (auto x : v) printf(" %lld", (long long)x); printf(" ;"); }
static void put_bits(const std::vector<double>& v) { for (double x : v) { uint64_t b; memcpy(&b, &x, 8); printf(" %llu", (unsigned long long)b); } printf(" ;"); }

int main() {
  std::string kind;
  while (std::cin >> kind) {
    if (kind != "F") return 3;
    long long nr, ne, nt; std::cin >> nr >> ne >> nt;
    const double thr = take_bits(1)[0];
    const auto off = take<int64_t>((size_t)nr + 1); const auto taxon = take<int32_t>((size_t)ne); const auto ident = take_bits((size_t)ne); const auto best = take<int64_t>((size_t)nr);
    const int code = mm::ident_args_check(nr, off.data(), taxon.data(), ident.data(), best.data(), nt, thr);
    if (code) { if (!*mm::ident_arg_message(code)) return 2; printf("refused %d\n", code); continue; }
    mm::IdentHostOut o;
    mm::ident_filter_host(nr, off.data(), taxon.data(), ident.data(), best.data(), nt, thr, &o);
    put_bits(o.sorted_max); printf(" %lld ;", (long long)o.n_le); put(o.taxon_reads); put_bits(o.taxon_median); put(o.taxon_removed); put(o.read_removed);
    put(o.read_src); put(o.entry_src); put(o.read_off_out);
    printf("\n");
  }
  return 0;
}
