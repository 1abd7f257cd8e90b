// CPU unit test of bgzip FASTA/FASTQ reading in the host program: SeqFile over the inflated segments of a BgzfStream (what the CLI does,
// with the device's segment inflater; here the host's) against SeqFile through zlib's gzread, the reader of every other gzip file.
//   t gz FILE | t bgzf FILE     one line per record: name, length, the sequence; then "end"
//   t detect FILE...            one line per file: "<is_bgzf_file> <is_bam_file>"
// A reader error prints "error: <message>" and exits 2.
#include "../metamaps_amd/csrc/host/seq_reader.hpp"
#include "../metamaps_amd/csrc/host/bam_reader.hpp"
#include <cstdio>

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: t gz|bgzf FILE | t detect FILE...\n"); return 1; }
  const std::string mode = argv[1];
  if (mode == "detect") {
    for (int i = 2; i < argc; ++i) printf("%d %d\n", bam::is_bgzf_file(argv[i]) ? 1 : 0, bam::is_bam_file(argv[i]) ? 1 : 0);
    return 0;
  }
  auto dump = [](SeqFile& f) {
    while (f.next()) {
      const std::string s = f.view ? std::string(f.view, f.view_len) : f.seq;
      printf("%s\t%zu\t%s\n", f.name.c_str(), s.size(), s.c_str());
    }
    printf("end\n");
  };
  try {
    if (mode == "gz") { SeqFile f(argv[2]); dump(f); }
    else {
      bam::BgzfStream z(argv[2], 1, nullptr, false);
      SeqFile f([&](std::vector<unsigned char>& buf) -> size_t {
        while (!z.at_end()) if (const size_t n = z.inflate_segment(buf, 0)) return n;
        return 0;
      });
      dump(f);
    }
  } catch (const bam::Error& e) {
    printf("error: %s\n", e.what());
    return 2;
  }
  return 0;
}
