// Host driver of metamaps_amd/csrc/host/reads_out.hpp (tests/test_reads_out_host.py).
//   opts key=value ...     the command line's options through reads_out_options: "on on on on | with_qual | tokens of --extract-taxa | tokens of --deplete-taxa", or
//                          the message and exit 1
//   select key=value ...   stdin: the contig names on the first line, the reads' line offsets on the second, then per line of PREFIX "contig field14": the
//                          primary contig of every read (-1: none) on one line, then per file that is on "label: the reads it takes"
//   scan PATH key=value    check_reference_taxa over the FASTA (plain or gzip) at PATH: "ok", or extract_taxon's message and exit 1
//   suffix                 the four files' suffixes with and without --base-qualities
#include "../metamaps_amd/csrc/host/reads_out.hpp"
#include <sstream>

static Options options_of(int argc, char** argv, int from) {
  Options o;
  for (int i = from; i < argc; ++i) { const std::string a = argv[i]; const size_t e = a.find('='); o.v[a.substr(0, e)] = e == std::string::npos ? "1" : a.substr(e + 1); }
  return o;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "suffix") {
    for (int f = 0; f < N_EXTRACT; ++f) printf("%s %s %s\n", kExtract[f].flag, side_suffix(kExtract[f].side, true).c_str(), side_suffix(kExtract[f].side, false).c_str());
    const Options none;
    Options both; both.v["extract-mapped"] = "1"; both.v["paf"] = "1";
    Options only; only.v["deplete-taxa"] = "9";
    printf("%d %d %d %d %d\n", reads_out_asked(none) ? 1 : 0, reads_out_asked(both) ? 1 : 0, side_files_of(both)[SIDE_EDIT] ? 1 : 0, reads_out_asked(only) ? 1 : 0,
           side_files_of(only)[SIDE_EDIT] ? 1 : 0);
    return 0;
  }
  if (mode == "scan" && argc > 2) { check_reference_taxa(reads_out_options(options_of(argc, argv, 3)), argv[2]); printf("ok\n"); return 0; }
  if (mode != "opts" && mode != "select") { fprintf(stderr, "usage: test_reads_out_host opts|select|suffix ...\n"); return 2; }
  const ReadsOutOpts r = reads_out_options(options_of(argc, argv, 2));
  if (mode == "opts") {
    printf("%d %d %d %d | %d |", r.on[0], r.on[1], r.on[2], r.on[3], r.with_qual ? 1 : 0);
    for (const std::string& t : r.list[EX_TAXA]) printf(" %s", t.c_str());
    printf(" |");
    for (const std::string& t : r.list[EX_DEPLETED]) printf(" %s", t.c_str());
    printf("\n");
    return 0;
  }
  std::string line;
  std::getline(std::cin, line);
  std::vector<std::string> cname; { std::istringstream is(line); for (std::string s; is >> s;) cname.push_back(s); }
  std::getline(std::cin, line);
  std::vector<int64_t> off; { std::istringstream is(line); for (int64_t v; is >> v;) off.push_back(v); }
  std::vector<int32_t> contig; std::vector<double> q;
  while (std::getline(std::cin, line)) { std::istringstream is(line); int32_t c; std::string t; if (is >> c >> t) { contig.push_back(c); q.push_back(strtod(t.c_str(), nullptr)); } }
  const ContigHits h = contig_hits(r, cname);
  const std::vector<int32_t> primary = primary_contigs(off, contig, q);
  for (int32_t p : primary) printf("%d ", p);
  printf("\n");
  static const char* const label[N_EXTRACT] = {"unmapped", "mapped", "taxa", "depleted"};
  for (int f = 0; f < N_EXTRACT; ++f) {
    if (!r.on[(size_t)f]) continue;
    printf("%s:", label[f]);
    for (int32_t x : extract_selection(f, primary, h)) printf(" %d", x);
    printf("\n");
  }
  return 0;
}
