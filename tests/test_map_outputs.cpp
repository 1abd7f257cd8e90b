// CPU unit test of the text and byte rules of mapDirectly's side outputs: metamaps_amd/csrc/host/edit_dist.hpp, paf_out.hpp, bam_out.hpp and the table
// of the side files, side_files.hpp.  Nothing else of the program is included and nothing of the C ABI is called: no device.  The expected values are
// the Python side's (tests/test_map_outputs.py); this program only applies the code under test to the inputs it is given and prints what comes out.
//   edit                         the lines of .editDistances for two reads and three records (fixed below)
//   paf                          the lines of .paf for one unaligned record and one with the runs 5= 1X 2I 3D 4= on strand -
//   header [NAME LEN]...         bam_header of those contigs, raw, on stdout
//   mapq TEXT...                 a batch text with TEXT as field 14 of its lines, the last line without a newline -> bam_line_q + bam_mapq, one per line
//   fields (R NAMELEN | Q,DIST,STRAND)...   bam_fields of the reads so described (read r is named by NAMELEN times the letter 'a' + r, its records
//                                follow it; contig = record index mod 3): "read strand contig flag mapq name_end" per record, then the joined names
//   table FLAG...                the suffixes of the side files those options ask for, each followed by " bgzf" where the file is BGZF
//   eof                          the BGZF end-of-file block, raw, on stdout
// Built and run by tests/test_map_outputs.py with g++ -fsanitize=address,undefined (no GPU needed).
#include "../metamaps_amd/csrc/host/bam_out.hpp"
#include "../metamaps_amd/csrc/host/edit_dist.hpp"
#include "../metamaps_amd/csrc/host/paf_out.hpp"
#include "../metamaps_amd/csrc/host/side_files.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static mm_map_record record(int read, int contig, int strand) {
  mm_map_record x{};
  x.read = read; x.ref_contig = contig; x.strand = strand;
  return x;
}

static int edit() {
  const std::vector<std::string> names{"r1", "r2"}, cname{"cA", "cB"};
  const std::vector<int64_t> off{0, 2, 3};
  const std::vector<mm_map_record> rec{record(0, 0, 1), record(0, 1, -1), record(1, 1, -1)};
  const int32_t dist[3] = {3, -1, 0};
  const int64_t first[3] = {10, 0, 99}, last[3] = {58, 0, 148};
  std::string out = "stale";
  edit_distance_text(dist, first, last, names, off, rec, cname, out);
  fwrite(out.data(), 1, out.size(), stdout);
  return 0;
}

static int paf() {
  const std::vector<std::string> names{"q1"}, cname{"ctg"};
  const std::vector<int> lens{12}, clen{5000};
  const std::vector<int64_t> off{0, 2};
  const std::vector<mm_map_record> rec{record(0, 0, 1), record(0, 0, -1)};
  BatchAlignment A;
  A.dist = {-1, 6}; A.first = {0, 100}; A.last = {0, 112}; A.op_off = {0, 0, 5};
  A.ops = {5u << 4 | 7u, 1u << 4 | 8u, 2u << 4 | 1u, 3u << 4 | 2u, 4u << 4 | 7u};
  std::string out = "stale";
  paf_text(A, names, lens, off, rec, cname, clen, out);
  fwrite(out.data(), 1, out.size(), stdout);
  return 0;
}

static int header(int argc, char** argv) {
  std::vector<std::string> cname; std::vector<int> clen;
  for (int i = 2; i + 1 < argc; i += 2) { cname.push_back(argv[i]); clen.push_back(atoi(argv[i + 1])); }
  const std::string h = bam_header(cname, clen);
  fwrite(h.data(), 1, h.size(), stdout);
  return 0;
}

static int mapq(int argc, char** argv) {
  std::string text;
  for (int i = 2; i < argc; ++i) { text += "read 10 0 9 + contig "; text += argv[i]; if (i + 1 < argc) text += '\n'; }
  for (double q : bam_line_q(text, (size_t)(argc - 2))) printf("%d\n", (int)bam_mapq(q));
  return 0;
}

static int fields(int argc, char** argv) {
  std::vector<std::string> names; std::vector<int64_t> off; std::vector<mm_map_record> rec; std::vector<int32_t> dist; std::string text;
  for (int i = 2; i < argc; ++i) {
    if (!strcmp(argv[i], "R") && i + 1 < argc) { off.push_back((int64_t)rec.size()); names.emplace_back((size_t)atoi(argv[++i]), (char)('a' + names.size())); continue; }
    char q[64]; int d = 0, s = 0;
    if (names.empty() || sscanf(argv[i], "%63[^,],%d,%d", q, &d, &s) != 3) { fprintf(stderr, "bad record %s\n", argv[i]); return 2; }
    rec.push_back(record((int)names.size() - 1, (int)(rec.size() % 3), s));
    dist.push_back(d);
    text += "line of "; text += q; text += ' '; text += q; text += '\n';
  }
  off.push_back((int64_t)rec.size());
  const BamFields F = bam_fields(dist, rec, names, off, text);
  for (size_t i = 0; i < rec.size(); ++i)
    printf("%d %d %d %u %u %lld\n", F.read[i], F.strand[i], F.contig[i], (unsigned)F.flag[i], (unsigned)F.mapq[i], (long long)F.name_off[i + 1]);
  printf("%lld %s\n", (long long)F.name_off[0], F.all_names.c_str());
  return 0;
}

static int table(int argc, char** argv) {
  Options o;
  for (int i = 2; i < argc; ++i) o.v[argv[i]] = "1";
  const SideSet on = side_files_of(o);
  for (int s = 0; s < N_SIDE; ++s) if (on[(size_t)s]) printf("%s%s\n", kSideFiles[s].suffix, kSideFiles[s].bgzf ? " bgzf" : "");
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "edit") return edit();
  if (mode == "paf") return paf();
  if (mode == "header") return header(argc, argv);
  if (mode == "mapq") return mapq(argc, argv);
  if (mode == "fields") return fields(argc, argv);
  if (mode == "table") return table(argc, argv);
  if (mode == "eof") { fwrite(kBgzfEof, 1, sizeof kBgzfEof, stdout); return 0; }
  fprintf(stderr, "usage: test_map_outputs edit|paf|header|mapq|fields|table|eof ...\n");
  return 2;
}
