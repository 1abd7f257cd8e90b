// Every MM_* environment switch the library and the drop-in CLI read, in ONE place (round-4 review: 68 switches, 14 of them documented).  None is
// needed to run the product: defaults are what bench.py and the tests' main paths use.  Kinds:
//   user     a knob a deployment may turn (sizes of batches, worker counts, progress output)
//   tuning   a measured threshold between two code paths whose results are identical either way
//   test     a hook that forces a rarely taken — or a cross-check — path so that the tests can hold it against the default path / the oracle;
//            results are identical, speed is not
//   debug    traces and timing aids (stderr output, early kernel exits that RETURN NO RESULTS: never set outside tools/)
// MM_STRICT_ENV=1 makes mm_ctx_create (and the CLI at start) refuse any MM_* variable that is not in this table: a misspelt switch is an
// error instead of a silent default.  tests/test_env_table.py holds the table against the sources and INTEGRATION.md against the table.
#pragma once
#include <unistd.h>
#include <cstdlib>
#include <cstring>
#include <string>

extern "C" char** environ;

namespace mm {

struct EnvSwitch { const char* name; const char* dflt; const char* kind; const char* what; };

inline const EnvSwitch* env_table(size_t* n) {
  static const EnvSwitch T[] = {
    {"MM_STRICT_ENV", "unset", "user", "refuse MM_* variables that are not in this table (mm_ctx_create returns MM_ERR_ARG, the CLI exits 1)"},
    {"MM_CPU_BUDGET", "min(hardware threads, affinity mask, cgroup CPU quota)", "user", "CPUs the process may keep busy: what every thread pool of the library and the CLI is sized from (cpu_budget.hpp)"},
    {"MM_SYNC", "block when the CPU budget is <= 32, else spin", "user", "how a host thread waits for its stream: \"spin\" (hipStreamSynchronize) or \"block\" (sleep on an event created with hipEventBlockingSync)"},
    // ---- CLI (host/metamaps_main.cpp, host/*.hpp)
    {"MM_CLI_WORKERS", "4", "user", "worker contexts per GPU that take read batches in turn (= --workers-per-gpu)"},
    {"MM_CLI_BATCH_READS", "100000", "user", "reads per batch handed to a worker"},
    {"MM_CLI_BATCH_MBASES", "256", "user", "... or this many million bases, whichever comes first"},
    {"MM_CLI_MAP_SLOTS", "2", "tuning", "batches per device that may be inside their mapping section at the same time"},
    {"MM_CLI_BLOCK_BYTES", "128 MiB", "tuning", "block size of the block-parallel FASTQ/FASTA parser over an mmap-ed query file"},
    {"MM_CLI_REF_BLOCK_BYTES", "min(group, 256 MiB)", "tuning", "the same for the reference FASTA"},
    {"MM_CLI_REF_GROUP_BASES", "2^30", "test", "bases per upload group of the reference (small groups: the concat path on small inputs)"},
    {"MM_CLI_REF_SEQUENTIAL", "unset", "test", "reference through the sequential kseq-style reader instead of the block parser"},
    {"MM_BAM_HOST_DECODE", "unset", "test", "BAM query files decoded to ASCII on the host and uploaded like FASTQ (cross-check of the device nt16 packer)"},
    {"MM_BGZF_HOST_INFLATE", "unset", "test", "BGZF query files (BAM, bgzip FASTA/FASTQ) inflated by zlib on the host, never on the device (cross-check of mm_bgzf_inflate)"},
    {"MM_BAM_DEVICE_INFLATE", "unset", "tuning", "BAM query files inflated on the device (mm_bgzf_inflate) instead of by zlib on the host's threads: a third of the host CPU, slower on 16 CPUs (DESIGN.md §1)"},
    {"MM_CLI_NO_MMAP", "unset", "test", "plain query and reference files through the sequential reader instead of the memory-mapped block parser (what pipes and, with MM_GZIP_HOST_INFLATE, plain gzip take)"},
    {"MM_GZIP_HOST_INFLATE", "unset", "test", "plain gzip query and reference files inflated by zlib's sequential reader on the host, never on the device (cross-check of mm_gzip_*)"},
    {"MM_GZIP_CHUNK_BYTES", "262144", "test", "compressed bytes per speculatively decoded chunk of a plain gzip stream (mm_gzip_open with chunk_bytes 0): small values make small files run through many chunks"},
    {"MM_DEFLATE_HOST", "unset", "test", "mm_bgzf_deflate (the mappings file of --compress-output) writes its BGZF members with zlib level 1 on the host's threads instead of the device kernel: the A/B partner and a fallback; other bytes, the same text"},
    {"MM_CLI_NO_PREWARM", "unset", "test", "worker contexts come up with their first batch instead of beside the index build"},
    {"MM_SF_GRID", "the device's CU count", "debug", "resident workgroups of the streaming seed filter (measurement aid: how K3 scales with the CUs at work)"},
    {"MM_CLI_LATE_READER", "unset", "debug", "the query reader starts when the index is built instead of beside the build (measurement aid)"},
    {"MM_CLI_NO_SKETCH_REUSE", "unset", "test", "chunk-major runs recompute minimizers and sketches per chunk (mm_map_batch instead of mm_map_batch_reusing)"},
    {"MM_CLI_NO_HUGE", "unset", "test", "no transparent-huge-page arena for host blocks >= 4 MiB (huge_new.hpp)"},
    {"MM_CLI_FULL_TEARDOWN", "unset", "test", "destroy every object and run static destructors at exit instead of _exit after the last file is closed"},
    {"MM_CLASSIFY_THREADS", "32", "user", "host threads that tokenise the mappings file and format classify's outputs"},
    {"MM_EM_MAX_ITER", "unbounded", "test", "cap on EM iterations in classify (the reference has none)"},
    {"MM_EM_SLICE", "1024", "test", "EM iterations per mm_em_run / mm_em_continue call of classify"},
    {"MM_CLI_TIMING", "unset", "debug", "phase laps of the CLI on stderr (bench.py's e2e legs parse them)"},
    {"MM_CLI_FORMAT_TRACE", "unset", "debug", "per-thread times of the text formatting of a batch on stderr"},
    // ---- library: allocator (mm_alloc.hpp)
    {"MM_DEVICE_BYTES_CAP", "0 (off)", "test", "the library behaves as if every device had this many bytes: allocations beyond fail, mm_ctx_device_info reports it (placement tests)"},
    {"MM_INDEX_SCALE_MB", "8192", "test", "blocks from this size on are index-scale (pooled per device); a few MB exercise the pool on small inputs"},
    {"MM_NO_SLABS", "unset", "test", "worker buffers are not cut out of pooled index-scale blocks"},
    {"MM_NO_POOL_RESCUE", "unset", "test", "round-3 behaviour: a request the driver refuses hands the whole pool back instead of being served from it"},
    {"MM_ALLOC_TRACE", "unset", "debug", "every block that comes from the driver, with its cost, on stderr"},
    {"MM_CTX_TRACE", "unset", "debug", "phases of mm_ctx_create (HIP initialisation, stream, allocator) on stderr"},
    {"MM_HOST_TIMING", "unset", "debug", "host-side sections of mm_map_batch and of the index build on stderr"},
    {"MM_PACK_SCALAR", "unset", "test", "mm_seqset_upload packs bases with the byte-table loop only (cross-check of the AVX2 path, host_pack.cpp)"},
    // ---- library: index build (mm_index.hip)
    {"MM_INDEX_PART_MAX", "2^31 - 2^24 entries", "test", "entries per partition of the hash sort (small values: the partitioned sort + merge on small inputs)"},
    {"MM_DUP_SAT", "65535", "test", "saturation value of the stored same-hash neighbour distances (small values: K5's scan fall-back)"},
    // ---- library: mapping (mm_map.hip, mm_seq.hip)
    {"MM_EAGER_TIEBREAK", "unset", "test", "resolve every duplicate-hash strand by the reference's std::sort order up front instead of only where a strand vote reads one"},
    {"MM_FORCE_AMB_REDO", "unset", "test", "every read with an unresolved strand goes through the redo path"},
    {"MM_NO_HIT_FILTER", "unset", "test", "K3 without the exact seed-hit pre-filter: every hit of every kept list reaches the sort (parity tests of the raw hit list)"},
    {"MM_NO_FUSED_FILTER", "unset", "test", "K3 as probe_kernel + two-pass hit_filter_kernel for every read (what reads that do not fit the fused kernel take)"},
    {"MM_HF_STAGE_CAP", "auto", "test", "capacity of a read's survivor stage (tiny values: the overflow / re-filter path)"},
    {"MM_HF_WIDE_FROM", "13000", "tuning", "sketch size from which the two-pass filter counts in 32768 position slots instead of 8192"},
    {"MM_SEGSORT_MAX_KEYS", "2^32 - 1", "test", "keys per call of K4's segmented device sort (small values: the split on small inputs)"},
    {"MM_L1_SERIAL", "unset", "test", "K4's L1 merge loop as the literal one-thread-per-read loop (cross-check of the wavefront form)"},
    {"MM_L2_FULL", "unset", "test", "K5 evaluates every window (the literal slide) instead of the exact skip-ahead"},
    {"MM_L2_DENSE_FROM", "13000", "tuning", "sketch size from which K5 runs as l2_codes_kernel + l2_dense_kernel"},
    {"MM_L2_DENSE_NO_STOP", "unset", "test", "dense path without its early stop (every window evaluated)"},
    {"MM_L2_NO_SMALL_GROUPS", "unset", "test", "groups of fewer than three candidates also run as four-wave workgroups (one launch instead of two)"},
    {"MM_L2_HOST_GROUPS", "unset", "test", "candidate groups formed on the host instead of by l2_group_kernel"},
    {"MM_L2_NO_GROUP_SORT", "unset", "test", "K5 workgroups in read order instead of the order of their candidates' positions"},
    {"MM_L2_GROUP_SORT_MIN", "2048", "tuning", "groups from which the launch order is sorted"},
    {"MM_L2_V1", "unset", "test", "every candidate below 32 768 sketch hashes that is not on the dense path through l2_kernel's wide form (one wave per candidate) instead of the zone kernel l2z_kernel (mm_l2z.hpp), no device grouping: the cross-check"},
    {"MM_L2_V1_LONG", "unset", "test", "only the long-read classes B and D (sketches of 3 073 .. 13 000 hashes) through l2_kernel's wide form, the 10 kb class through the zone kernel"},
    {"MM_L2_NO_FUSE", "unset", "test", "zone kernel without the band predicted from L1's seed-hit count: its masks always come from a second pass over the stream"},
    {"MM_L2_NO_RANGES", "unset", "test", "the zone kernel's waves search their candidates' index ranges themselves (until round 6) instead of taking them from l2_ranges_kernel (cross-check)"},
    {"MM_L2Z_FORCE_HANDBACK", "unset", "test", "the zone kernel hands every candidate that reaches its band loop to l2_kernel, as its pass-count guard does (the hand-back path against the default)"},
    {"MM_L2Z_WALK_SEARCH", "unset", "test", "the 10 kb zone kernel finds the next block to sweep by the walk one block at a time (the long-read classes' way) instead of by ballots: the same blocks, the cross-check"},
    {"MM_L2Z_DBG", "unset", "debug", "zone kernel writes pivot-minus-estimate and its pass count INSTEAD OF RESULTS (tools/l2z_pivot_hist.py; 2: against the predicted estimate)"},
    {"MM_L2_ONE_STREAM", "unset", "test", "the two launches of K5's 10 kb class one behind the other on the context's stream instead of side by side (auxiliary stream)"},
    {"MM_L2_NO_SLOTS", "unset", "test", "K5 scratch indexed by wave number of the launch instead of per-XCD slots taken and given back"},
    {"MM_L2_SLOTS", "auto (resident waves)", "tuning", "number of K5 scratch slots"},
    {"MM_L2_STOP", "0", "debug", "K5 leaves after phase n WITHOUT RESULTS (tools/l2_stop.py)"},
    {"MM_L2_PHASES", "unset", "debug", "K5 phase clocks into its counters (tools/l2_long_phases.py; the zone kernel has them in a build with -DL2Z_CLOCKS only)"},
    {"MM_MZ_DBG", "0", "debug", "K1 leaves after step n WITHOUT RESULTS (tools/stage_ms.py)"},
    {"MM_HF_DBG", "0", "debug", "two-pass filter leaves after phase n WITHOUT RESULTS"},
    {"MM_SF_PROF", "unset", "debug", "cycle counts per phase of the streaming seed filter on stderr"},
    // ---- library: EM and exchange (mm_post.hip, mm_api.hip)
    {"MM_EM_FORCE_COLLECTIVE", "unset", "test", "a one-rank communicator keeps P1-P3' | ncclAllReduce | finalize instead of P1-P3 alone (how one GPU drives the multi-rank path)"},
    {"MM_EM_GRID", "by size", "tuning", "workgroups of the EM kernels; by default enough for about 160 reads and 448 mappings each, 256 at least, one per read at most; when set: at most 1024 and one per 256 reads"},
    // ---- library: gene-level analysis (mm_gene.hip)
    {"MM_GENE_PAIR_BUDGET", "2^26", "test", "(mapping, gene) pairs, feature keys and median keys per tile of mm_gene_overlap (small values: many tiles on small inputs; no result depends on it)"},
    {"MM_GENE_TIMING", "unset", "debug", "device times of mm_gene_overlap's stages (events) on stderr (tools/gene_kernel_stats.py)"},
    // ---- library: identity filter (mm_ident.hip)
    {"MM_IDENT_TIMING", "unset", "debug", "device times of mm_ident_filter's stages (events) on stderr (tools/ident_filter_stats.py)"},
    // ---- library: edit distances (mm_edit.hip)
    {"MM_EDIT_TIMING", "unset", "debug", "device times of the job and alignment stages of mm_mapping_edit_distances / mm_edit_infix, and of the trace stage of mm_mapping_align / mm_edit_infix_align with its scratch budget and launches (events) on stderr (tools/edit_kernel_stats.py)"},
    {"MM_EDIT_TRACE_MB", "an eighth of the device's free memory at the call", "tuning", "scratch of one launch of the alignment trace (mm_mapping_align, mm_edit_infix_align) in MiB: the jobs are cut into launches that fit it, one job at least per launch; no result depends on it"},
    {"MM_BAM_TIMING", "unset", "debug", "device times of the upload, size, scan, write and deflate stages of mm_bam_encode (events; deflate includes the members' copy to the host) with its jobs, records, runs, groups, raw and BGZF bytes on stderr (tools/edit_kernel_stats.py --bam)"},
    {"MM_BAM_SORT_TIMING", "unset", "debug", "device times of every window of mm_bam_sorter_window: inflate (with the members' upload), gather, deflate (with the members' copy to the host), with the members inflated and the bytes, on stderr (tools/edit_kernel_stats.py --bam-sort)"},
    {"MM_PILEUP_TIMING", "unset", "debug", "device times of mm_pileup_events' upload, count, scan, emit, sort and reduce stages (events; reduce includes the table's copy to the host) with its jobs, runs, events, pairs and fetched bytes, and of the stages of mm_pileup_merge and mm_pileup_finish, on stderr (tools/edit_kernel_stats.py --pileup)"},
    {"MM_PILEUP_MERGE_PAIRS", "64 * 2^20", "test", "mapDirectly --pileup: (key, count) pairs a query file's accumulator may hold before it is replaced by its mm_pileup_merge (small values: several merges on small runs; no result depends on it)"},
    {"MM_VCF_TIMING", "unset", "debug", "device times of mm_vcf_events' upload, count, scan, emit, sort and reduce stages (events; reduce includes the table's copy to the host) with its jobs, runs, events, indels, pairs and fetched bytes, and of the stages of mm_vcf_merge and mm_vcf_finish, on stderr (tools/edit_kernel_stats.py --vcf)"},
    {"MM_VCF_MERGE_PAIRS", "64 * 2^20", "test", "mapDirectly --vcf: (w0, w1, count) triples a query file's accumulator may hold before it is replaced by its mm_vcf_merge (small values: several merges on small runs; no result depends on it)"},
    {"MM_MODS_TIMING", "unset", "debug", "device times of the modification plane's upload and kernel in mm_seqset_upload with its groups, calls and staged bytes, of mm_mod_events' upload, count, scan, emit, sort and reduce stages (events; reduce includes the table's copy to the host) with its jobs, runs, events, pairs and fetched bytes, and of the stages of mm_mod_merge and mm_mod_finish, and of mm_mod_motifs' scan, sites and order stages with the group's contig range, tiles, entries, listed contigs, motifs and rows, on stderr"},
    {"MM_MODS_MERGE_PAIRS", "64 * 2^20", "test", "mapDirectly --mods: (key, count) pairs a query file's accumulator may hold before it is replaced by its mm_mod_merge (small values: several merges on small runs; no result depends on it)"},
    {"MM_CONS_TIMING", "unset", "debug", "device times of mm_consensus' intervals, candidates, select, positions, offsets and emit stages (emit includes the text's copy to the host) with the group's contig range, bases, entries, intervals, kept rows, written contigs and text bytes, on stderr (tools/edit_kernel_stats.py --consensus)"},
    {"MM_DEPTH_TIMING", "unset", "debug", "device times of mm_depth_profile's intervals, breakpoints, runs, contigs and windows stages (each includes its results' copy to the host) with its intervals, unique breakpoints, runs, listed contigs and windows, on stderr (tools/edit_kernel_stats.py --depth)"},
    {"MM_BAM_SORT_WINDOW_MB", "255", "tuning", "mapDirectly --bam-sorted: MiB of sorted records the merge makes at a time (mm_bam_sorter_create's window_bytes), rounded down to whole members of 65 280 bytes, one member at least (0), 255 MiB at most; device memory of the merge is two windows; no file depends on it"},
    {"MM_READS_OUT_TIMING", "unset", "debug", "device times of the upload, size, scan, write and deflate stages of mm_reads_encode (events; deflate includes the members' copy to the host) with its records, record kind, groups, raw and BGZF bytes on stderr (tools/edit_kernel_stats.py --reads-out)"},
    {"MM_ERRPROF_TIMING", "unset", "debug", "device times of mm_errprof_events' upload, check, walk and sum stages (sum includes the results' copy to the host) with its jobs, runs and workgroups, and of mm_errprof_finish's sort and rows stages with its entries and listed contigs, on stderr (tools/edit_kernel_stats.py --error-profile)"},
    {"MM_ERRPROF_GROUPS", "16 per CU", "test", "mm_errprof_events: workgroups of the walk, each with its counters in LDS and one row of partial sums, grid-stride over the jobs (never more than the jobs or 65536; 1 or 3: a workgroup walks many jobs on small inputs; no result depends on it)"},
    {"MM_CONS_GROUP_BASES", "2^28", "test", "mapDirectly --consensus: reference bases one mm_consensus call may cover; consecutive contigs are grouped up to it and a longer contig is a group alone (small values: one call per contig on small runs; no result depends on it)"},
    {"MM_MOTIF_GROUP_BASES", "2^28", "test", "mapDirectly --mod-motifs: reference bases one mm_mod_motifs call may cover; consecutive contigs are grouped up to it and a longer contig is a group alone (small values: one call per contig on small runs; no result depends on it)"},
    {"MM_CLI_FORMAT_PART", "10000", "test", "mapping records per formatter thread of a batch (the text of a batch is formatted in up to eight parts and joined)"},
    {"MM_CLI_CLASSIFY_FROM_FILE", "unset", "test", "mapDirectly --then-classify reads PREFIX back and tokenises it (as `classify` does) instead of taking the lines it has just formatted from memory"},
    {"MM_GATHER_SELF_SEND", "unset", "test", "mm_mapping_gather sends the owner's own parts through ncclSend / ncclRecv too (one-GPU test of the exchange)"},
  };
  *n = sizeof T / sizeof T[0];
  return T;
}

// names of MM_* variables in the environment that the table does not know ("" when all are known)
inline std::string env_unknown() {
  size_t n = 0; const EnvSwitch* T = env_table(&n);
  std::string bad;
  for (char** e = environ; e && *e; ++e) {
    if (strncmp(*e, "MM_", 3) != 0) continue;
    const char* eq = strchr(*e, '=');
    const std::string name(*e, eq ? (size_t)(eq - *e) : strlen(*e));
    // switches of the repository's own Python / shell side (bench.py, tests/, tools/): read there, not by the product — a fuzz campaign or an
    // A/B run (MM_LIB_PATH) must be combinable with strict mode.  tests/test_env_table.py holds this list against *.py and *.sh.
    static const char* const outside[] = {"MM_BENCH_", "MM_FUZZ_", "MM_TEST_", "MM_CLI_FUZZ_CASES", "MM_LIB_PATH"};
    bool ours = false;
    for (const char* pfx : outside) ours = ours || name.rfind(pfx, 0) == 0;
    if (ours) continue;
    bool known = false;
    for (size_t i = 0; i < n && !known; ++i) known = name == T[i].name;
    if (!known) bad += (bad.empty() ? "" : ", ") + name;
  }
  return bad;
}
inline bool env_strict() { const char* e = getenv("MM_STRICT_ENV"); return e && *e && strcmp(e, "0") != 0; }

}  // namespace mm
