// Host driver of metamaps_amd/csrc/host/motif_out.hpp (tests/test_motif_out.py).
//   opts key=value ...   the command line's options through mods_options and motif_options: "n min_frac combine | LETTERS:pos masks.. | ...", or the message and exit 1
//   rc LETTERS           1 where the motif is its own reverse complement as a sequence of letter sets, else 0
//   text key=value ...   stdin: contig names on the first line, then rows "R site motif code n_mod n_canonical n_other n_fail" and summary entries
//                        "S contig motif code sites covered modified n_valid_cov n_mod", cut into groups by lines "G": PREFIX.motifs.bedmethyl, a line "==", and
//                        PREFIX.motifs.tsv to stdout, made group by group as map_outputs.hpp does
#include "../metamaps_amd/csrc/host/motif_out.hpp"
#include <sstream>

static Options options_of(int argc, char** argv, int from) {
  Options o;
  for (int i = from; i < argc; ++i) { const std::string a = argv[i]; const size_t e = a.find('='); o.v[a.substr(0, e)] = e == std::string::npos ? "1" : a.substr(e + 1); }
  return o;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "rc" && argc > 2) { printf("%d\n", motif_own_reverse_complement(argv[2]) ? 1 : 0); return 0; }
  if (mode != "opts" && mode != "text") { fprintf(stderr, "usage: test_motif_out opts|rc|text ...\n"); return 2; }
  const Options o = options_of(argc, argv, 2);
  const ModsOpts mo = mods_options(o);
  const MotifOpts mt = motif_options(o, mo);
  if (mode == "opts") {
    printf("%d %g %d", mt.on ? mt.n : 0, mt.min_frac, mt.combine ? 1 : 0);
    for (int k = 0; k < mt.n; ++k) {
      printf(" | %s:%d", mt.text[k].c_str(), mt.pos[(size_t)k]);
      for (int32_t i = mt.off[(size_t)k]; i < mt.off[(size_t)k + 1]; ++i) printf(" %d", (int)mt.mask[(size_t)i]);
    }
    printf("\n");
    return 0;
  }
  std::string line;
  std::getline(std::cin, line);
  std::istringstream names(line);
  std::vector<std::string> cname; for (std::string s; names >> s;) cname.push_back(s);
  std::string bed, tsv = motif_tsv_header();
  std::vector<int64_t> total;
  std::vector<uint64_t> site, a, b, c, d; std::vector<int32_t> motif, code, s_contig, s_motif, s_code; std::vector<int64_t> sums;
  auto group = [&] {
    motif_bedmethyl_text(mo, mt, site, motif, code, a, b, c, d, cname, bed);
    motif_tsv_text(mo, mt, s_contig, s_motif, s_code, sums, cname, total, tsv);
    for (auto* v : {&site, &a, &b, &c, &d}) v->clear();
    for (auto* v : {&motif, &code, &s_contig, &s_motif, &s_code}) v->clear();
    sums.clear();
  };
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind; in >> kind;
    if (kind == "G") group();
    else if (kind == "R") { unsigned long long s, w, x, y, z; int m, k; in >> s >> m >> k >> w >> x >> y >> z; site.push_back(s); motif.push_back(m); code.push_back(k); a.push_back(w); b.push_back(x); c.push_back(y); d.push_back(z); }
    else if (kind == "S") { int cc, m, k; long long v; in >> cc >> m >> k; s_contig.push_back(cc); s_motif.push_back(m); s_code.push_back(k); for (int x = 0; x < mmt::SUMS; ++x) { in >> v; sums.push_back(v); } }
  }
  motif_tsv_totals(mo, mt, total, tsv);
  fwrite(bed.data(), 1, bed.size(), stdout); printf("==\n"); fwrite(tsv.data(), 1, tsv.size(), stdout);
  return 0;
}
