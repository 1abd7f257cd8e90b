// CPU unit test of the command line program's device-free host code: CliSwitches (metamaps_amd/csrc/host/cli_switches.hpp) and the arithmetic of
// `classify` (metamaps_amd/csrc/host/taxonomy.hpp).  Nothing else of the program is included: no C ABI, no device.
//   test_cli_units self TAXDIR    the checks below, against the five-node taxonomy the Python side wrote into TAXDIR; "ok" and exit 0, or the failed lines and exit 1
//   test_cli_units binom          "n p k" lines on stdin -> "binomial_cdf(n, p, k) reg_inc_beta(k + 1, n - k, p)" per line, 17 significant digits
// Built and run by tests/test_cli_units.py with g++ -fsanitize=address,undefined (no GPU needed).
#include "../metamaps_amd/csrc/host/cli_switches.hpp"
#include "../metamaps_amd/csrc/host/taxonomy.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static int failed = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); ++failed; } } while (0)

static const char* const kSwitches[] = {"MM_CLI_TIMING", "MM_CLI_FULL_TEARDOWN", "MM_CLI_BATCH_READS", "MM_CLI_BATCH_MBASES", "MM_BGZF_HOST_INFLATE", "MM_BAM_DEVICE_INFLATE",
    "MM_BAM_HOST_DECODE", "MM_GZIP_HOST_INFLATE", "MM_CLI_NO_MMAP", "MM_CLI_BLOCK_BYTES", "MM_CLI_LATE_READER", "MM_CLI_REF_GROUP_BASES", "MM_CLI_REF_SEQUENTIAL",
    "MM_CLI_REF_BLOCK_BYTES", "MM_CLI_WORKERS", "MM_CLI_NO_PREWARM", "MM_CLI_MAP_SLOTS", "MM_CLI_NO_SKETCH_REUSE", "MM_CLI_FORMAT_PART", "MM_CLI_FORMAT_TRACE",
    "MM_CLI_CLASSIFY_FROM_FILE", "MM_CLASSIFY_THREADS", "MM_EM_MAX_ITER", "MM_EM_SLICE"};
static void clear_env() { for (const char* n : kSwitches) unsetenv(n); }

static void switches() {
  clear_env();
  {
    const CliSwitches sw;                                        // the defaults of the table in INTEGRATION.md
    CHECK(!sw.timing && !sw.full_teardown && !sw.bgzf_host_inflate && !sw.bam_device_inflate && !sw.bam_host_decode && !sw.gzip_host_inflate && !sw.no_mmap);
    CHECK(!sw.late_reader && !sw.ref_sequential && !sw.no_prewarm && !sw.no_sketch_reuse && !sw.format_trace && !sw.classify_from_file);
    CHECK(sw.batch_reads == 100000 && sw.batch_bases == 256000000LL);
    CHECK(sw.block_bytes == (size_t)128 << 20);
    CHECK(sw.ref_group_bases == (uint64_t)1 << 30 && sw.ref_block_bytes == (size_t)256 << 20);
    CHECK(sw.workers == 4 && sw.map_slots == 2 && sw.format_part == 10000);
    CHECK(sw.classify_threads == 0 && sw.em_max_iter == LLONG_MAX && sw.em_slice == 1024);
  }
  for (const char* n : {"MM_CLI_TIMING", "MM_CLI_NO_MMAP", "MM_BAM_DEVICE_INFLATE", "MM_BAM_HOST_DECODE", "MM_GZIP_HOST_INFLATE", "MM_CLI_CLASSIFY_FROM_FILE"}) setenv(n, "1", 1);
  setenv("MM_CLI_FULL_TEARDOWN", "", 1);                         // a flag counts when it is set, whatever it holds
  setenv("MM_CLI_BATCH_READS", "0", 1); setenv("MM_CLI_BATCH_MBASES", "3", 1); setenv("MM_CLI_WORKERS", "-5", 1); setenv("MM_CLI_MAP_SLOTS", "7", 1);
  setenv("MM_CLI_BLOCK_BYTES", "4096", 1); setenv("MM_CLI_FORMAT_PART", "junk", 1);
  setenv("MM_CLI_REF_GROUP_BASES", "5000000000", 1);             // beyond 32 bits: read with stoull
  setenv("MM_CLASSIFY_THREADS", "1000", 1); setenv("MM_EM_MAX_ITER", "3", 1); setenv("MM_EM_SLICE", "0", 1);
  {
    const CliSwitches sw;
    CHECK(sw.timing && sw.full_teardown && sw.no_mmap && sw.bam_device_inflate && sw.bam_host_decode && sw.gzip_host_inflate && sw.classify_from_file);
    CHECK(!sw.bgzf_host_inflate && !sw.late_reader && !sw.format_trace);
    CHECK(sw.batch_reads == 1 && sw.batch_bases == 3000000LL && sw.workers == 1 && sw.map_slots == 7);
    CHECK(sw.block_bytes == 4096 && sw.format_part == 1);
    CHECK(sw.ref_group_bases == 5000000000ull && sw.ref_block_bytes == (size_t)256 << 20);   // the block's default: the smaller of the group and 256 MiB
    CHECK(sw.classify_threads == 256 && sw.em_max_iter == 3 && sw.em_slice == 1);
  }
  setenv("MM_BGZF_HOST_INFLATE", "1", 1);                        // host inflate of every BGZF file wins over the device inflate of BAM
  setenv("MM_CLI_REF_GROUP_BASES", "1000", 1); setenv("MM_CLASSIFY_THREADS", "0", 1);
  {
    const CliSwitches sw;
    CHECK(sw.bgzf_host_inflate && !sw.bam_device_inflate);
    CHECK(sw.ref_group_bases == 1000 && sw.ref_block_bytes == 1000 && sw.classify_threads == 1);
  }
  setenv("MM_CLI_REF_BLOCK_BYTES", "7", 1);
  { const CliSwitches sw; CHECK(sw.ref_block_bytes == 7); }
  clear_env();
}

// 1 root -> 2 Bacteria (superkingdom) -> 10 Escherichia (genus) -> 100 Escherichia coli (species) -> x7 (a strain node of the database builder)
static void taxonomy(const std::string& dir) {
  const Taxonomy T(dir);
  CHECK(T.T.size() == 5);
  CHECK(T.T.at("100").parent == "10" && T.T.at("100").rank == "species" && T.T.at("100").sci == "Escherichia coli");
  CHECK(T.first_non_x("x7") == "100" && T.first_non_x("100") == "100" && T.first_non_x("1") == "1");
  const auto up = T.upward_by_ranks("x7", {"species", "genus", "family"});
  CHECK(up.size() == 3 && up.at("species") == "100" && up.at("genus") == "10" && up.at("family") == "Undefined");
  const auto f = Taxonomy::fields(" 9\t|\tsome  name\t|\t\t|\tscientific name\t|");
  CHECK(f.size() == 5 && f[0] == " 9" && f[1] == "some  name" && f[2].empty() && f[3] == "scientific name" && f[4].empty());
  CHECK(extract_taxon("NC_000913.3|kraken:taxid|100|Escherichia") == "100");
  CHECK(extract_taxon("kraken:taxid|x7|c1") == "x7");
  CHECK(extract_taxon("kraken:taxid|none kraken:taxid|12") == "12");   // the first occurrence that carries digits
  // the WIMP's frequencies go up the tree: both genomes end in species 100, genus 10
  const auto W = wimp_em_frequencies(T, {{"x7", 0.25}, {"100", 0.75}}, {{"x7", 1}});
  CHECK(W.at("definedGenomes").emF.at("x7") == 0.25 && W.at("definedGenomes").emF.at("100") == 0.75);
  CHECK(W.at("species").emF.size() == 1 && W.at("species").emF.at("100") == 1.0 && W.at("genus").emF.at("10") == 1.0 && W.at("family").emF.at("Undefined") == 1.0);
}

// one contig of 2 500 bases: three windows of 1 000, the last one short
static void coverage() {
  ContigCoverage C;
  C.add("100", "c1", 2500, 100, 1299);                           // 900 bases of window 0, 300 of window 1
  C.add("100", "c1", 2500, 2000, 2600);                          // ends beyond the contig: cut to its last base, 500 bases of window 2
  const std::vector<size_t>& v = C.cov.at("100").at("c1");
  const std::vector<size_t>& n = C.reads.at("100").at("c1");
  CHECK(v.size() == 3 && v[0] == 900 && v[1] == 300 && v[2] == 500);
  CHECK(n.size() == 3 && n[0] == 1 && n[1] == 1 && n[2] == 1);
  CHECK(C.last.at("100").at("c1") == (size_t)2500 - (size_t)3000);   // the length of a short last window as the reference computes it (fEM.h:744: it wraps)
  ContigCoverage D;
  D.add("100", "c2", 3000, 0, 2999);                             // a multiple of the window: every window full
  CHECK(D.cov.at("100").at("c2") == std::vector<size_t>({1000, 1000, 1000}) && D.last.at("100").at("c2") == 1000);
  D.add("100", "c3", 400, 10, 19);
  CHECK(D.cov.at("100").at("c3") == std::vector<size_t>({10}) && D.last.at("100").at("c3") == 400);
}

static void mapq() {
  CHECK(mapq_as_classify_reads_it("1", 1) == 1.0);
  CHECK(mapq_as_classify_reads_it("0.5", 3) == 0.5);
  CHECK(mapq_as_classify_reads_it("1e-05", 5) == 1e-05);
  CHECK(mapq_as_classify_reads_it("0.5 next", 3) == 0.5);         // the length counts, not a terminator
  CHECK(mapq_as_classify_reads_it("1e-320", 6) == 0.0);           // a denormal: the reference takes 0 (fEM.h:269-275)
  CHECK(binomial_cdf(10, 0.5, 10) == 1 && binomial_cdf(10, 0, 3) == 1 && binomial_cdf(10, 1, 3) == 0);
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "binom")) {
    double n, p, k;
    while (scanf("%lf %lf %lf", &n, &p, &k) == 3) printf("%.17g %.17g\n", binomial_cdf(n, p, k), reg_inc_beta(k + 1, n - k, p));
    return 0;
  }
  if (argc != 3 || strcmp(argv[1], "self")) return 2;
  switches();
  taxonomy(argv[2]);
  coverage();
  mapq();
  if (failed) return 1;
  printf("ok\n");
  return 0;
}
