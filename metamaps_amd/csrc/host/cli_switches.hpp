// Every MM_* environment switch the command line program reads (huge_new.hpp's MM_CLI_NO_HUGE apart: operator new cannot wait for main), each
// parsed ONCE into a const member with its default beside it.  One instance is made in main and passed by reference.  Reading once is right here
// where it is not in the library (mm_map.hip's MapSwitches is made per call): a run of the CLI is one process with one environment, nothing sets
// a switch between two batches.  INTEGRATION.md carries the table of all switches (mm_env.hpp); the standard library only in here.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <string>

namespace {

struct CliSwitches {
  static bool on(const char* e) { return e != nullptr; }
  static int at_least_1(const char* e, int dflt) { return e ? std::max(1, atoi(e)) : dflt; }
  static long long num(const char* e, long long dflt) { return e ? atoll(e) : dflt; }
  static uint64_t u64(const char* e, uint64_t dflt) { return e ? std::stoull(e) : dflt; }
  // both sub-commands
  const bool timing = on(getenv("MM_CLI_TIMING"));               // wall time per phase on stderr at exit, and a line per lap, batch and worker
  const bool full_teardown = on(getenv("MM_CLI_FULL_TEARDOWN")); // the orderly way out instead of _exit: the tests of handle lifetimes under a leak checker
  // the reader of the query files
  const int64_t batch_reads = at_least_1(getenv("MM_CLI_BATCH_READS"), 100000);   // (test hook, small batches)
  const int64_t batch_bases = (int64_t)at_least_1(getenv("MM_CLI_BATCH_MBASES"), 256) * 1000000LL;   // ~0.25 Gbp per device batch (16 ms of mapping)
  const bool bgzf_host_inflate = on(getenv("MM_BGZF_HOST_INFLATE"));   // bgzip text through zlib's sequential gz reader instead of mm_bgzf_inflate
  const bool bam_device_inflate = !bgzf_host_inflate && on(getenv("MM_BAM_DEVICE_INFLATE"));   // a BAM's blocks on the device too (default: the host's TaskPool)
  const bool bam_host_decode = on(getenv("MM_BAM_HOST_DECODE")); // a BAM's 4-bit codes decoded to ASCII on the host instead of mm_seqset_add_nt16
  const bool gzip_host_inflate = on(getenv("MM_GZIP_HOST_INFLATE"));   // plain gzip (queries and the reference) through zlib's sequential reader instead of mm_gzip_*
  const bool no_mmap = on(getenv("MM_CLI_NO_MMAP"));             // plain files (queries and the reference) through the sequential reader too
  const size_t block_bytes = (size_t)at_least_1(getenv("MM_CLI_BLOCK_BYTES"), 128 << 20);   // block of the query files' block-parallel parser
  const bool late_reader = on(getenv("MM_CLI_LATE_READER"));     // measurement aid: the reader starts when the index is built
  // the reference
  const uint64_t ref_group_bases = u64(getenv("MM_CLI_REF_GROUP_BASES"), (uint64_t)1 << 30);   // (test hook: small groups)
  const bool ref_sequential = on(getenv("MM_CLI_REF_SEQUENTIAL"));
  const size_t ref_block_bytes = (size_t)at_least_1(getenv("MM_CLI_REF_BLOCK_BYTES"), (int)std::min<uint64_t>(ref_group_bases, (uint64_t)256 << 20));
  // mapping
  const size_t workers = (size_t)at_least_1(getenv("MM_CLI_WORKERS"), 4);       // worker contexts per device (--workers-per-gpu goes first)
  const bool no_prewarm = on(getenv("MM_CLI_NO_PREWARM"));
  const size_t map_slots = (size_t)at_least_1(getenv("MM_CLI_MAP_SLOTS"), 2);   // batches per device inside their mapping section at a time
  const bool no_sketch_reuse = on(getenv("MM_CLI_NO_SKETCH_REUSE"));            // chunk-major modes: sketches recomputed per chunk (the cross-check)
  const size_t format_part = (size_t)at_least_1(getenv("MM_CLI_FORMAT_PART"), 10000);   // records per formatting part (tests: several parts for small batches too)
  const bool format_trace = on(getenv("MM_CLI_FORMAT_TRACE"));
  const size_t pileup_merge_pairs = (size_t)u64(getenv("MM_PILEUP_MERGE_PAIRS"), (uint64_t)64 << 20);   // --pileup: pairs above which a file's accumulator is merged (tests: small)
  const size_t vcf_merge_pairs = (size_t)u64(getenv("MM_VCF_MERGE_PAIRS"), (uint64_t)64 << 20);   // --vcf: the same for its (w0, w1, count) triples
  const size_t mods_merge_pairs = (size_t)u64(getenv("MM_MODS_MERGE_PAIRS"), (uint64_t)64 << 20);   // --mods: the same for its (key, count) pairs
  const int64_t cons_group_bases = (int64_t)std::clamp<uint64_t>(u64(getenv("MM_CONS_GROUP_BASES"), (uint64_t)1 << 28), 1, (uint64_t)1 << 40);   // --consensus: bases per call
  const int64_t motif_group_bases = (int64_t)std::clamp<uint64_t>(u64(getenv("MM_MOTIF_GROUP_BASES"), (uint64_t)1 << 28), 1, (uint64_t)1 << 40);   // --mod-motifs: the same
  // --bam-sorted: output bytes the merge makes at a time, whole members of 65 280 bytes (unset: 0, the library's 255 MiB; 0 MB: one member)
  const int64_t bam_sort_window = !getenv("MM_BAM_SORT_WINDOW_MB") ? 0 : (int64_t)std::clamp<uint64_t>((u64(getenv("MM_BAM_SORT_WINDOW_MB"), 0) << 20) / 65280, 1, 4096) * 65280;
  const bool classify_from_file = on(getenv("MM_CLI_CLASSIFY_FROM_FILE"));      // --then-classify reads the mappings file back instead of taking the kept lines
  // classify
  const int classify_threads = std::min(256, at_least_1(getenv("MM_CLASSIFY_THREADS"), 0));   // pieces of the tokeniser and the output formatter (tests); 0: by the size of the input
  const long long em_max_iter = num(getenv("MM_EM_MAX_ITER"), LLONG_MAX);   // (test hook; the reference has no cap)
  const int em_slice = at_least_1(getenv("MM_EM_SLICE"), 1024);  // iterations per device-resident call (test hook)
};

}  // namespace
