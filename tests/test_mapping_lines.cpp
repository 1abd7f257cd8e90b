// CPU unit test of the device-free half of `classify` (metamaps_amd/csrc/host/mapping_lines.hpp, classify_tables.hpp; clean_frequencies of taxonomy.hpp).
// The two headers alone are included, so it compiles without the device's C ABI.  Built and run by tests/test_mapping_lines.py with g++: plain, with
// -fsanitize=address,undefined and with -fsanitize=thread (the tokeniser and its join run on threads).  No GPU needed.
//   parse FILE DB N   FILE tokenised in N pieces, then (if it has a line) the tables of FILE.meta and DB/taxonInfo.txt and the per-mapping fields:
//                       off O0 O1 ...
//                       contigs ID ...                      (in the order they were interned)
//                       taxa ID ...
//                       L readID n last_space contigID len start stop ident mapq taxon inv        (one per line; doubles as %.17g)
//   adopt FILE DB     the same lines handed over as KeptLines in two parts (contig names in another order, reads without lines between), same print
//   shards            em_shard for reads 0, 1, 5 over G = 1, 2, 3, 8:   NR G d lo hi e0 soff...
//   stats V...        bootstrap_row_stats:   mean sd lo hi
//   clean N ID=F[:R]...   clean_frequencies with N mapped reads, R best mappings of ID (0: none):   ID=F ...
#include "../metamaps_amd/csrc/host/classify_tables.hpp"
#include "../metamaps_amd/csrc/host/mapping_lines.hpp"
#include <cstdio>

static void read_into(const std::string& fn, TextBuf& text) {
  std::ifstream s(fn, std::ios::binary);
  if (!s.is_open()) die("cannot open " + fn);
  const std::string all((std::istreambuf_iterator<char>(s)), std::istreambuf_iterator<char>());
  text.resize(all.size());
  memcpy(text.p, all.data(), all.size());
}

static void print(const MappingLines& M, const std::string& mapped, const std::string& db) {
  printf("off"); for (int64_t o : M.off) printf(" %lld", (long long)o); printf("\n");
  if (M.off.size() - 1 != M.NRD) die("NRD is not the number of reads");
  printf("contigs"); for (auto& c : M.contig_id) printf(" %s", c.c_str()); printf("\n");
  for (size_t c = 0; c < M.contig_id.size(); ++c) if (M.contig_index.at(M.contig_id[c]) != (int)c) die("contig_index does not invert contig_id");
  if (M.lines.empty()) return;
  ClassifyTables C = read_tables(M, mapped, db);
  per_mapping_fields(M, C);
  printf("taxa"); for (auto& t : C.taxa) printf(" %s", t.c_str()); printf("\n");
  for (size_t i = 0; i < M.lines.size(); ++i) {
    const MapLine& L = M.lines[i];
    const std::string_view id = read_id(L);
    printf("L %.*s %u %u %s %lld %zu %zu %.17g %.17g %d %.17g\n", (int)id.size(), id.data(), L.n, L.last_space, M.contig_id[(size_t)L.contig].c_str(), L.len, L.start, L.stop,
           L.ident, L.mapq, (int)C.taxon[i], C.inv[i]);
    if (C.mapq[i] != L.mapq) die("the EM's mapq is not the line's");
  }
}

// the lines of M (tokenised from T0) as mapDirectly would have kept them: two parts, the contigs numbered by `cname`, a read without lines at the start, in
// the middle and at the end of each part
static void adopt_mode(const char* T0, const MappingLines& M, const std::string& mapped, const std::string& db) {
  std::vector<std::string> cname(M.contig_id.rbegin(), M.contig_id.rend());
  cname.insert(cname.begin(), "kraken:taxid|1|never_mapped");
  std::map<std::string, int32_t> cnum; for (size_t c = 0; c < cname.size(); ++c) cnum[cname[c]] = (int32_t)c;
  const size_t half = M.NRD / 2;
  std::vector<LineMeta> meta[2]; std::vector<int64_t> off[2];
  KeptLines K; K.cname = &cname;
  for (int part = 0; part < 2; ++part) {
    const size_t r0 = part ? half : 0, r1 = part ? M.NRD : half, l0 = (size_t)M.off[r0], l1 = (size_t)M.off[r1];
    const char* const base = l0 < M.lines.size() ? M.lines[l0].p : T0;
    for (size_t i = l0; i < l1; ++i) {
      const MapLine& L = M.lines[i];
      meta[part].push_back(LineMeta{(uint32_t)(L.p - base), L.last_space, L.n, cnum.at(M.contig_id[(size_t)L.contig]), (int32_t)L.len, (int32_t)L.start, (int32_t)L.stop, L.ident, L.mapq});
    }
    off[part].push_back(0); off[part].push_back(0);                // a read without lines first
    for (size_t r = r0; r < r1; ++r) {
      off[part].push_back(M.off[r + 1] - (int64_t)l0);
      if (r == r0 + (r1 - r0) / 2) off[part].push_back(off[part].back());   // and one in the middle
    }
    off[part].push_back(off[part].back());                        // and one at the end
    K.parts.push_back(KeptLines::Part{base, meta[part].data(), meta[part].size(), off[part].data(), off[part].size() - 1});
  }
  print(adopt(K), mapped, db);
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if ((mode == "parse" && argc == 5) || (mode == "adopt" && argc == 4)) {
    TextBuf text; read_into(argv[2], text);
    const MappingLines M = tokenise(text.c_str(), text.size(), mode == "parse" ? (size_t)atoi(argv[4]) : 1, argv[2]);
    if (mode == "parse") print(M, argv[2], argv[3]); else adopt_mode(text.c_str(), M, argv[2], argv[3]);
    return 0;
  }
  if (mode == "shards") {
    for (size_t NR : {0, 1, 5}) for (size_t G : {1, 2, 3, 8}) {
      std::vector<int64_t> off{0}; for (size_t r = 0; r < NR; ++r) off.push_back(off.back() + 1 + (int64_t)(r * 7 % 4));   // 1 to 4 mappings per read
      for (size_t d = 0; d < G; ++d) {
        const EmShard s = em_shard(off, G, d);
        printf("%zu %zu %zu %zu %zu %zu", NR, G, d, s.lo, s.hi, s.e0); for (int64_t o : s.soff) printf(" %lld", (long long)o); printf("\n");
        if (s.e0 != (size_t)off[s.lo]) die("e0 is not the shard's first mapping");
        for (size_t i = 0; i + 1 < s.soff.size(); ++i) if (s.soff[i + 1] - s.soff[i] != off[s.lo + i + 1] - off[s.lo + i]) die("soff does not keep the reads' sizes");
      }
    }
    return 0;
  }
  if (mode == "stats" && argc > 3) {
    std::vector<double> v; for (int i = 2; i < argc; ++i) v.push_back(strtod(argv[i], nullptr));
    const RowStats s = bootstrap_row_stats(v);
    printf("%.17g %.17g %.17g %.17g\n", s.mean, s.sd, s.lo, s.hi);
    return 0;
  }
  if (mode == "clean" && argc > 3) {
    std::map<std::string, double> f; std::map<std::string, size_t> reads;
    for (int i = 3; i < argc; ++i) {
      const std::vector<std::string> kv = split(argv[i], "="), fr = split(kv.at(1), ":");
      f[kv.at(0)] = strtod(fr.at(0).c_str(), nullptr);
      if (fr.size() > 1 && fr[1] != "0") reads[kv[0]] = (size_t)strtoull(fr[1].c_str(), nullptr, 10);
    }
    clean_frequencies(f, reads, (size_t)strtoull(argv[2], nullptr, 10));
    for (auto& e : f) printf("%s=%.17g ", e.first.c_str(), e.second);
    printf("\n");
    return 0;
  }
  die("usage: parse FILE DB N | adopt FILE DB | shards | stats V... | clean N ID=F[:R]...");
}
