// Host driver of metamaps_amd/csrc/host/mods_out.hpp and of bam_reader.hpp's aux walk (tests/test_mods_out.py).
//   opts key=value ...   the command line's options through mods_options: "n_codes base:name ... min_ml min_coverage", or its message and exit 1
//   bam FILE LIST        every record of FILE read with want_tags: "name l_seq | mm type:bytes | ml type:sub:count | mn value-or-none | RESULT" with RESULT
//                        "none", "groups: base code mode n skip.. ml.. / ..." or "error: message"; a last line with the file's counters
//   text LIST            stdin: contig names on the first line, then rows "site n_mod n_canonical n_other n_fail": PREFIX.bedmethyl to stdout
#include "../metamaps_amd/csrc/host/mods_out.hpp"
#include <sstream>

static Options options_of(int argc, char** argv, int from) {
  Options o;
  for (int i = from; i < argc; ++i) { const std::string a = argv[i]; const size_t e = a.find('='); o.v[a.substr(0, e)] = e == std::string::npos ? "1" : a.substr(e + 1); }
  return o;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "opts") {
    const ModsOpts m = mods_options(options_of(argc, argv, 2));
    printf("%d", m.on ? m.n_codes : 0);
    for (int k = 0; k < m.n_codes; ++k) printf(" %c:%s", m.code_base[k], m.code_name[k].c_str());
    printf(" %d %lld\n", m.min_ml, m.min_coverage);
    return 0;
  }
  if (mode == "bam" && argc > 3) {
    Options o; o.v["mods"] = argv[3];
    const ModsOpts m = mods_options(o);
    ModGroups g; ModCounters n;
    try {
      bam::Reader br(argv[2], 1, (1LL << 29) - 1, true, nullptr, true);
      bam::Record r;
      while (br.next(r)) {
        printf("%s %lld | mm %c:%zu | ml %c:%c:%zu | mn %s | ", r.name.c_str(), (long long)r.l_seq, r.mm.type ? r.mm.type : '-', r.mm.bytes, r.ml.type ? r.ml.type : '-', r.ml.sub ? r.ml.sub : '-',
               r.ml.count * (r.ml.type != 0), r.mn.type && strchr("cCsSiI", r.mn.type) ? std::to_string(bam::aux_int(r.mn)).c_str() : "none");
        try {
          ++n.reads;
          if (!mods_parse(m, r.mm, r.ml, r.mn, r.l_seq, g, n)) { printf("none\n"); continue; }
          ++n.with_tags;
          printf("groups:");
          for (size_t k = 0; k < g.base.size(); ++k) {
            printf("%s %c %d %d %lld", k ? " /" : "", g.base[k], (int)g.code[k], (int)g.mode[k], (long long)(g.off[k + 1] - g.off[k]));
            for (int64_t j = g.off[k]; j < g.off[k + 1]; ++j) printf(" %u", g.skips[(size_t)j]);
            for (int64_t j = g.off[k]; j < g.off[k + 1]; ++j) printf(" %u", (unsigned)g.ml[(size_t)j]);
          }
          printf("\n");
        } catch (const ModTagError& e) { printf("error: %s\n", e.what()); }
      }
    } catch (const bam::Error& e) { printf("bam error: %s\n", e.what()); return 0; }
    printf("counters %zu %zu %zu %zu %zu\n", n.reads, n.with_tags, n.minus_groups, n.n_groups, n.mn_mismatch);
    return 0;
  }
  if (mode == "text" && argc > 2) {
    Options o; o.v["mods"] = argv[2];
    const ModsOpts m = mods_options(o);
    std::string line;
    std::getline(std::cin, line);
    std::istringstream names(line);
    std::vector<std::string> cname; for (std::string s; names >> s;) cname.push_back(s);
    std::vector<uint64_t> site, a, b, c, d;
    for (unsigned long long s, w, x, y, z; std::cin >> s >> w >> x >> y >> z;) { site.push_back(s); a.push_back(w); b.push_back(x); c.push_back(y); d.push_back(z); }
    const std::string t = bedmethyl_text(m, site, a, b, c, d, cname);
    fwrite(t.data(), 1, t.size(), stdout);
    return 0;
  }
  fprintf(stderr, "usage: test_mods_out opts|bam|text ...\n");
  return 2;
}
