// CPU unit test of the text rules of mapDirectly --depth, metamaps_amd/csrc/host/depth_out.hpp, compiled on its own: nothing else of the program is included
// and nothing of the C ABI is called.  The expected values are the Python side's (tests/test_depth_out.py).
//   text [KEY VALUE]...   the three texts of a small profile under those options, each behind a line "== name"
//   opts [KEY VALUE]...   what those options give: "on window T1,T2,..." (or the program ends with status 1 and a message)
#include "../metamaps_amd/csrc/host/depth_out.hpp"
#include <cstdio>

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  Options o;
  for (int i = 2; i + 1 < argc; i += 2) o.v[argv[i]] = argv[i + 1];
  const DepthOpts p = depth_options(o);
  if (mode == "opts") {
    printf("%d %lld ", (int)p.on, p.window);
    for (int k = 0; k < p.n_thresholds; ++k) printf("%s%lld", k ? "," : "", (long long)p.thresholds[k]);
    printf("\n");
    return 0;
  }
  if (mode == "text") {                                            // contigs cA (7 bases, no alignment), kraken:taxid|9|cB (2500), cC (3); the counters of tests/test_depth_out.py
    const std::vector<std::string> cname{"cA", "kraken:taxid|9|cB", "cC"};
    const std::vector<int> clen{7, 2500, 3};
    const std::vector<int64_t> win_off{0, 3, 4};
    const size_t per = (size_t)(mmdp::STATS + p.n_thresholds);
    std::vector<int64_t> stats(2 * per, 0);
    const int64_t b[5] = {3, 1700, 4100, 1, 4}, c[5] = {70000, 3, 210000, 70000, 70000};
    for (int k = 0; k < 5; ++k) { stats[(size_t)k] = b[k]; stats[per + (size_t)k] = c[k]; }
    for (int k = 0; k < p.n_thresholds; ++k) { stats[5 + (size_t)k] = 1700 - 100 * k; stats[per + 5 + (size_t)k] = 3; }
    std::string t = "== bedgraph\n" + depth_bedgraph_text({1, 1, 2}, {0, 1000, 0}, {1000, 1700, 3}, {1, 4, 70000}, cname);
    t += "== windows\n" + depth_windows_text({1, 2}, win_off, {1000, 2800, 0, 210000}, {1000, 700, 0, 3}, p.window, cname, clen);
    t += "== contigs\n" + depth_contigs_text(p, {1, 2}, stats, cname, clen);
    t += "== empty\n" + depth_bedgraph_text({}, {}, {}, {}, cname) + depth_windows_text({}, {0}, {}, {}, p.window, cname, clen) + depth_contigs_text(p, {}, {}, cname, clen);
    fwrite(t.data(), 1, t.size(), stdout);
    return 0;
  }
  fprintf(stderr, "usage: test_depth_out text|opts [KEY VALUE]...\n");
  return 2;
}
