// CPU unit test of the host program's BAM reader (metamaps_amd/csrc/host/bam_reader.hpp), driven by tests/test_bam_reader.py.
//   t detect FILE...                 one line per file: 1 if it is taken for BAM, else 0
//   t read FILE THREADS [all] [MAX]  one line per record: name, l_seq, flag, the 4-bit code bytes in hex, the read as sequenced;
//                                    then "blocks N eof E"; a reader error prints "error: <message>" and exits 2
//   t rate FILE THREADS              the reader's rate: records, bases, seconds, compressed MB/s, inflated MB/s (tools/bam_cli_bench.py)
#include "../metamaps_amd/csrc/host/bam_reader.hpp"
#include <sys/stat.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: t detect FILE... | t read FILE THREADS [all] [MAX]\n"); return 1; }
  const std::string mode = argv[1];
  if (mode == "detect") {
    for (int i = 2; i < argc; ++i) printf("%d\n", bam::is_bam_file(argv[i]) ? 1 : 0);
    return 0;
  }
  const unsigned threads = argc > 3 ? (unsigned)atoi(argv[3]) : 1;
  const bool all = argc > 4 && std::string(argv[4]) == "all";
  const int64_t max_len = argc > 5 ? atoll(argv[5]) : (1LL << 29) - 1;
  if (mode == "rate") {
    const auto t0 = std::chrono::steady_clock::now();
    int64_t n = 0, bases = 0, bytes = 0;
    bam::Reader br(argv[2], threads, max_len);
    bam::Record r;
    while (br.next(r)) { ++n; bases += r.l_seq; bytes += 36 + (int64_t)r.name.size() + (r.l_seq + 1) / 2 + r.l_seq; }   // (fixed fields + name + seq + qual)
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    struct stat st; stat(argv[2], &st);
    printf("records %lld bases %lld seconds %.3f compressed_MBps %.1f inflated_MBps %.1f\n", (long long)n, (long long)bases, s, st.st_size / s / 1e6, bytes / s / 1e6);
    return 0;
  }
  try {
    bam::Reader br(argv[2], threads, max_len, !all);
    bam::Record r;
    std::string hex, ascii;
    static const char* H = "0123456789abcdef";
    while (br.next(r)) {
      const size_t nb = ((size_t)r.l_seq + 1) / 2;
      hex.resize(2 * nb);
      for (size_t i = 0; i < nb; ++i) { hex[2 * i] = H[r.seq[i] >> 4]; hex[2 * i + 1] = H[r.seq[i] & 15]; }
      ascii.resize((size_t)r.l_seq);
      bam::nt16_to_ascii(r.seq, (size_t)r.l_seq, r.reverse(), &ascii[0]);
      printf("%s\t%lld\t%u\t%s\t%s\n", r.name.c_str(), (long long)r.l_seq, (unsigned)r.flag, hex.c_str(), ascii.c_str());
    }
    printf("blocks %zu eof %d\n", br.blocks(), br.eof_marker() ? 1 : 0);
  } catch (const bam::Error& e) {
    printf("error: %s\n", e.what());
    return 2;
  }
  return 0;
}
