// CPU unit test of the text rules of mapDirectly --pileup, metamaps_amd/csrc/host/pileup_out.hpp, compiled on its own: nothing else of the program is included
// and nothing of the C ABI is called.  The expected values are the Python side's (tests/test_pileup_out.py).
//   text                       PREFIX.pileup and, behind a line "--", PREFIX.pileup.contigs for the sites and contigs fixed below
//   use FLAG,DIST...           pileup_use of those records, one 0 / 1 per line
//   opts [KEY VALUE]...        the thresholds those options give: "on min_count min_frac" (or the program ends with status 1 and a message)
#include "../metamaps_amd/csrc/host/pileup_out.hpp"
#include <cstdio>
#include <cstring>

static int text() {
  const std::vector<std::string> cname{"cA", "kraken:taxid|9|cB", "cC"};
  const std::vector<int> clen{100, 4000000, 7};
  const std::vector<uint64_t> key{mmp::make_key(0, 0, 1), mmp::make_key(0, 99, 5), mmp::make_key(1, 3999999, 6), mmp::make_key(1, 3999999, 4), mmp::make_key(2, 3, 3)};
  const std::string a = pileup_text(key, {3, 12, 4000000000u, 1, 2}, {3, 40, 4000000001u, 9, 2}, {'A', 'N', 'g', 'T', 'C'}, cname);
  const std::string b = pileup_contigs_text({6, 0, 1}, {51, 0, 7}, {65, 0, 5000000000ll}, cname, clen);
  fwrite(a.data(), 1, a.size(), stdout); puts("--"); fwrite(b.data(), 1, b.size(), stdout);
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "text") return text();
  if (mode == "use") {
    std::vector<uint16_t> flag; std::vector<int32_t> dist;
    for (int i = 2; i < argc; ++i) { unsigned f = 0; int d = 0; if (sscanf(argv[i], "%u,%d", &f, &d) != 2) return 2; flag.push_back((uint16_t)f); dist.push_back(d); }
    for (uint8_t u : pileup_use(flag, dist)) printf("%d\n", (int)u);
    return 0;
  }
  if (mode == "opts") {
    Options o;
    for (int i = 2; i + 1 < argc; i += 2) o.v[argv[i]] = argv[i + 1];
    const PileupOpts p = pileup_options(o);
    printf("%d %lld %.17g\n", (int)p.on, p.min_count, p.min_frac);
    return 0;
  }
  fprintf(stderr, "usage: test_pileup_out text|use|opts ...\n");
  return 2;
}
