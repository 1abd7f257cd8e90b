// CPU unit test of the LCA assignment (metamaps_amd/csrc/mm_lca_core.hpp).  Commands on stdin, one answer line each:
//   T n parent[0..n)          "tree 0" if the tree is refused, else "tree 1" and three lines: depth, tin, tout (the later R lines use it)
//   H bits                    "thr 0|1": is the threshold (a double as its 64 bits, decimal) accepted
//   X n_nodes n t[0..n)       "taxa 0|1": are these taxon nodes inside a tree of n_nodes
//   R bits n (node bits)*n    "node bits": lca and mass of a read with these (node, posterior) entries at this threshold
// Built and run by tests/test_lca_core.py with g++, plain and with -fsanitize=address,undefined (no GPU needed).
#include "../metamaps_amd/csrc/mm_lca_core.hpp"
#include <cstdio>
#include <cstring>
#include <vector>

static double from_bits(unsigned long long b) { double d; memcpy(&d, &b, sizeof d); return d; }
static unsigned long long to_bits(double d) { unsigned long long b; memcpy(&b, &d, sizeof b); return b; }

int main() {
  std::vector<int32_t> parent, depth, tin, tout, node;
  std::vector<double> p;
  char cmd[4];
  while (scanf("%1s", cmd) == 1) {
    if (cmd[0] == 'T') {
      long long n; if (scanf("%lld", &n) != 1) return 2;
      parent.assign((size_t)(n > 0 ? n : 0), 0);
      for (auto& v : parent) if (scanf("%d", &v) != 1) return 2;
      const bool ok = mm::lca_tree_ok(n, parent.data());
      printf("tree %d\n", ok ? 1 : 0);
      if (!ok) continue;
      depth.assign((size_t)n, 0); tin.assign((size_t)n, 0); tout.assign((size_t)n, 0);
      mm::lca_derive(n, parent.data(), depth.data(), tin.data(), tout.data());
      for (const auto* a : {&depth, &tin, &tout}) { for (int32_t v : *a) printf("%d ", v); printf("\n"); }
    } else if (cmd[0] == 'H') {
      unsigned long long b; if (scanf("%llu", &b) != 1) return 2;
      printf("thr %d\n", mm::lca_threshold_ok(from_bits(b)) ? 1 : 0);
    } else if (cmd[0] == 'X') {
      long long nn, n; if (scanf("%lld %lld", &nn, &n) != 2) return 2;
      std::vector<int32_t> t((size_t)n);
      for (auto& v : t) if (scanf("%d", &v) != 1) return 2;
      printf("taxa %d\n", mm::lca_taxa_ok(n, t.data(), nn) ? 1 : 0);
    } else if (cmd[0] == 'R') {
      unsigned long long tb; long long n; if (scanf("%llu %lld", &tb, &n) != 2) return 2;
      node.resize((size_t)n); p.resize((size_t)n);
      for (long long k = 0; k < n; ++k) { unsigned long long b; if (scanf("%d %llu", &node[(size_t)k], &b) != 2) return 2; p[(size_t)k] = from_bits(b); }
      double mass = 0;
      const int32_t v = mm::lca_read(mm::LcaSerial{}, mm::LcaArrayEntries{node.data(), p.data(), tin.data()}, n,
                                     mm::LcaTree{tin.data(), tout.data(), parent.data()}, from_bits(tb), &mass);
      printf("%d %llu\n", v, to_bits(mass));
    } else return 2;
  }
  return 0;
}
