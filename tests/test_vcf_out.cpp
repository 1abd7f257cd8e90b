// CPU unit test of the text rules of mapDirectly --vcf, metamaps_amd/csrc/host/vcf_out.hpp, compiled on its own: nothing else of the program is included and
// nothing of the C ABI is called.  The expected values are the Python side's (tests/test_vcf_out.py).
//   header                     the header for three contigs
//   lines                      the lines of the alleles fixed below, one of every shape
//   opts [KEY VALUE]...        the thresholds those options give: "on min_count min_frac" (or the program ends with status 1 and a message)
#include "../metamaps_amd/csrc/host/vcf_out.hpp"
#include <cstdio>
#include <cstring>

static const std::vector<std::string> cname{"cA", "kraken:taxid|9|cB", "cC"};

static std::vector<uint8_t> windows(const std::vector<std::string>& w) {
  std::vector<uint8_t> out;
  for (const auto& s : w) { std::string t = s; t.resize((size_t)mmv::WINDOW, '\0'); out.insert(out.end(), t.begin(), t.end()); }
  return out;
}

static int lines() {
  const uint64_t L = (uint64_t)1 << mmv::LEN_SHIFT;
  // GAT: G 2 at bits 0, A 0 at bits 2, T 3 at bits 4
  const std::vector<uint64_t> w0{mmp::make_key(0, 0, 1), mmp::make_key(0, 9, mmp::CODE_DEL), mmp::make_key(0, 9, mmp::CODE_INS), mmp::make_key(0, 40, mmp::CODE_DEL),
                                 mmp::make_key(1, 3999999, mmp::CODE_INS), mmp::make_key(1, 3999999, 3), mmp::make_key(2, 2, mmp::CODE_DEL), mmp::make_key(2, 6, mmp::CODE_INS)};
  const std::vector<uint64_t> w1{0, 3, 3 * L | 2 | 0 << 2 | 3 << 4, 25, 30 * L, 0, 24, 24 * L | 0x1B1B1B1B1B1Bull};
  const std::string t = vcf_lines(w0, w1, {3, 12, 4, 5, 4000000000u, 1, 2, 7}, {3, 40, 40, 50, 4000000001u, 9, 2, 7},
                                  windows({"ACGT", "TrNA", "nCGT", "GACGTACGTACGTACGTACGTACGT", "c", "Y", "CAAAAAAAAAAAAAAAAAAAAAAAA", "G"}), cname);
  fwrite(t.data(), 1, t.size(), stdout);
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "header") { const std::string t = vcf_header(cname, {100, 4000000, 7}); fwrite(t.data(), 1, t.size(), stdout); return 0; }
  if (mode == "lines") return lines();
  if (mode == "opts") {
    Options o;
    for (int i = 2; i + 1 < argc; i += 2) o.v[argv[i]] = argv[i + 1];
    const VcfOpts p = vcf_options(o);
    printf("%d %lld %.17g\n", (int)p.on, p.min_count, p.min_frac);
    return 0;
  }
  fprintf(stderr, "usage: test_vcf_out header|lines|opts ...\n");
  return 2;
}
