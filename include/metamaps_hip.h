/*
 * metamaps_hip.h — C ABI of libmetamaps_hip.so, the MI355X (gfx950) implementation of the
 * MetaMaps mapping + EM-classification hot path.
 *
 * The reference (DiltheyLab/MetaMaps) has no FFI/plugin seam: its hot path is reached through
 * three in-process C++ interfaces (paths relative to /root/reference/src):
 *   (i)   skch::Sketch(param, maxMem, callback)            map/include/winSketch.hpp:157  — index one chunk
 *   (ii)  MapModuleOutput* skch::Map::mapModule(read)      map/include/computeMap.hpp:180 — map one read
 *   (iii) meta::doEM  per-read callback + reduction        meta/fEM.h:466, :535-600       — one EM iteration
 * Each entry point below names the interface (and the loops under it) that it replaces.  Handles are
 * opaque; buffers are caller-owned plain arrays; every call returns 0 on success or a negative
 * mm_status and leaves a message in mm_last_error().  No exceptions cross this boundary, no global
 * state.  A mm_ctx is one device + one stream + a scratch allocator; it and the objects created from it are used
 * from one host thread at a time, different contexts (one per GPU of a node, or several on one GPU) may be
 * driven from different threads concurrently, and an index may be read by mm_map_batch through any context of
 * the device it lives on.  There is no CPU fallback: mm_ctx_create fails when no gfx950 device is present.
 * A function that hands back a new handle through `out` (mm_seqset_hpc: through `out` and `map`) does so on MM_OK alone: on every
 * error *out is NULL and what the call had made is freed.
 */
#ifndef METAMAPS_HIP_H
#define METAMAPS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MM_ABI_VERSION 6   /* 3: mm_seqset_slice/concat, mm_map_batch_reusing, mm_em_continue, mm_synth_community_species;
                            * 4: mm_sketch_batch, mm_ctx_release_cached, mm_index_dup_neighbours;
                            * 5: mm_mapping_gather, mm_comm_info, mm_seqset_fetch_range;
                            * 6: mm_index_save, mm_index_load; mm_em_bootstrap, mm_gzip_*, mm_seqset_hpc + mm_hpc_map_* + mm_mapping_to_raw,
                            *    mm_em_lca, mm_gene_overlap, mm_ident_filter, mm_edit_infix + mm_mapping_edit_distances,
                            *    mm_edit_infix_align + mm_mapping_align + mm_alignment_*, mm_bam_* (mm_bam_encode_sorted, mm_bam_fetch_records, mm_bam_sorter_*), mm_pileup_*, mm_vcf_*, mm_consensus*, mm_seqset_*_mods, mm_mod_* (mm_mod_motifs, mm_motif_result_*), mm_reads_encode + mm_reads_text_*,
                            *    mm_depth_*, mm_errprof_* (additions to 6) */

typedef enum {
  MM_OK = 0,
  MM_ERR_ARG = -1,        /* bad argument / unsupported parameter value          */
  MM_ERR_DEVICE = -2,     /* HIP runtime error (message has the HIP error string) */
  MM_ERR_NOMEM = -3,      /* device or host allocation failed                     */
  MM_ERR_STATE = -4,      /* call sequence violated                               */
  MM_ERR_LIMIT = -5,      /* documented capacity limit exceeded       */
  MM_ERR_NUMERIC = -6,    /* reference would abort here (e.g. likelihood sum 0, mapWrap.h:298) */
  MM_ERR_COMM = -7,       /* RCCL error                                           */
  MM_ERR_DATA = -8        /* input data is corrupt (mm_bgzf_inflate: a block's status says which; mm_gzip_feed: the message names the offset) */
} mm_status;

typedef struct mm_ctx mm_ctx;          /* a device + streams + scratch allocator                  */
typedef struct mm_seqset mm_seqset;    /* sequences resident in HBM as packed 2-bit + exceptions  */
typedef struct mm_index mm_index;      /* reference sketch of one index chunk, resident in HBM     */
typedef struct mm_mapping mm_mapping;  /* mapping results of one read batch, resident in HBM      */
typedef struct mm_em mm_em;            /* EM state (mappings x taxa) resident in HBM              */
typedef struct mm_gzip mm_gzip;        /* a plain gzip stream being inflated on a context's device */
typedef struct mm_alignment mm_alignment;  /* base-level alignments (CIGAR runs) of a batch of jobs, in host memory */
typedef struct mm_reads_text mm_reads_text;   /* BGZF members holding FASTQ / FASTA records of selected reads, in host memory */
typedef struct mm_bam mm_bam;          /* BGZF members holding BAM records of a batch of jobs, in host memory */
typedef struct mm_bam_sorter mm_bam_sorter;  /* sorted runs of BAM records being merged into one coordinate-sorted stream on a context's device */
typedef struct mm_pileup mm_pileup;    /* a table of (key, count) pileup events, unique keys ascending, in host memory */
typedef struct mm_pileup_result mm_pileup_result;  /* the kept sites and the per-contig coverage of a run's pileup, in host memory */
typedef struct mm_vcf mm_vcf;          /* a table of (w0, w1, count) alleles, unique keys ascending, in host memory */
typedef struct mm_vcf_result mm_vcf_result;  /* the kept alleles of a run with their depths and reference windows, in host memory */
struct mm_consensus;                   /* the counters and the wrapped consensus text of a group of contigs, in host memory (no typedef: the entry
                                          point that makes one carries the name) */
typedef struct mm_hpc_map mm_hpc_map;  /* compressed -> raw coordinates of a homopolymer-compressed set, resident in HBM */

/* ---- context -------------------------------------------------------------------------------- */
int mm_abi_version(void);
int mm_device_count(void);                               /* visible HIP devices (0 when there is none or the runtime fails) */
int mm_ctx_create(int device_id, mm_ctx** out);
void mm_ctx_destroy(mm_ctx* ctx);
const char* mm_last_error(const mm_ctx* ctx);            /* valid until the next call on ctx       */
/* device name, CU count, total HBM bytes, free HBM bytes */
int mm_ctx_device_info(mm_ctx* ctx, char* name, size_t name_cap, int* cus, uint64_t* hbm_total, uint64_t* hbm_free);
int mm_ctx_synchronize(mm_ctx* ctx);
/* Hands the context's cached free device blocks, and the device's recycled index-scale blocks, back to the driver.  The library caches
 * what it frees (a context's own allocator; index-scale blocks per device) and gives it up by itself only when an allocation fails for
 * lack of memory; a host that has finished a phase — e.g. all chunk indexes of a --maxmemory run built, worker contexts about to start
 * beside them — calls this so that the memory is there without that detour. */
int mm_ctx_release_cached(mm_ctx* ctx);
/* raw hipStream_t the kernels are launched on (for event timing by the caller) */
void* mm_ctx_stream(mm_ctx* ctx);

/* ---- sequences -------------------------------------------------------------------------------
 * Replaces the kseq buffers handed to addMinimizers (commonFunc.hpp:92; callers winSketch.hpp:269,
 * computeMap.hpp:285).  Bytes are upper-cased exactly as makeUpperCase does (commonFunc.hpp:57);
 * A/C/G/T are packed 2 bits/base, every other byte is kept verbatim in an exception run list so that
 * hashing sees the same ASCII the reference hashes. */
int mm_seqset_create(mm_ctx* ctx, mm_seqset** out);
void mm_seqset_destroy(mm_seqset* s);
int mm_seqset_add(mm_seqset* s, const char* ascii, int64_t len);   /* host staging, keeps input order */
/* same, without the copy: the caller keeps `ascii` valid and unchanged until mm_seqset_upload has returned (a parser that
 * fills one arena per batch hands its records over this way) */
int mm_seqset_add_view(mm_seqset* s, const char* ascii, int64_t len);
/* BAM's packed form of a read: n_bases 4-bit codes of "=ACMGRSVTWYHKDBN", two per byte, the first in the high nibble (the `seq` field of a
 * BAM record, (n_bases + 1) / 2 bytes).  reverse != 0: the codes are the reverse complement of the read (BAM flag 0x10), which is stored
 * turned back — as `samtools fastq` writes it.  The set then holds what mm_seqset_add of that read in ASCII would give, byte for byte (codes
 * other than A/C/G/T become exception runs of their letter).  A view, like mm_seqset_add_view: `nt16` stays valid until mm_seqset_upload
 * has returned, which packs the codes on the device.  One set holds either ASCII or 4-bit sequences: adding the other kind is MM_ERR_STATE. */
int mm_seqset_add_nt16(mm_seqset* s, const uint8_t* nt16, int64_t n_bases, int reverse);
/* Base qualities, one byte per base beside the packed bases.  mm_seqset_add_qual attaches `len` quality bytes to the sequence added last (by
 * mm_seqset_add, _add_view or _add_nt16): offset 33 for the text of a FASTQ record, 0 for the raw Phred bytes of a BAM record; for an nt16 record
 * added with reverse != 0 the bytes are in the record's order and are turned back with the bases.  A view: `qual` stays valid and unchanged until
 * mm_seqset_upload has returned.  MM_ERR_ARG: no sequence yet, a second call for the same sequence, len other than that sequence's length, an
 * offset other than 0 or 33, a set that is uploaded.  A set may mix sequences with and without qualities.  mm_seqset_upload stages the bytes as it
 * does the bases and one kernel stores Phred 0..93 per base, 0xFF for a sequence without qualities; a byte outside [offset, offset + 93] is
 * MM_ERR_DATA, mm_last_error names the lowest such sequence and the byte.  A set without any mm_seqset_add_qual call allocates and launches
 * nothing for qualities.  mm_seqset_has_qual: 1 if any sequence of the set carries qualities.  mm_seqset_fetch_qual: the stored bytes of sequence i
 * in read order (cap >= its length), 0xFF each for a sequence without qualities.  mm_seqset_slice and mm_seqset_concat carry the qualities;
 * mm_seqset_save / _load and mm_seqset_hpc do not: their result has none. */
int mm_seqset_add_qual(mm_seqset* s, const uint8_t* qual, int64_t len, int offset);
int mm_seqset_has_qual(const mm_seqset* s);
int mm_seqset_fetch_qual(mm_seqset* s, int64_t i, uint8_t* out, int64_t cap);

/* Base modifications (the MM/ML tags of a read; SAM tags specification, "Base modifications"), two bytes per base beside the packed bases (DESIGN.md
 * section 1, "Base modifications"; the definition: csrc/mm_mods_core.hpp).  mm_seqset_add_mods attaches n_groups groups, in MM's order and one code
 * each, to the sequence added last (by mm_seqset_add, _add_view or _add_nt16): base[g] is one of 'A' 'C' 'G' 'T', code[g] the index 0..3 of the
 * group's code among the codes the caller asks for or -1 for any other code, mode[g] is '.', '?' or 0 for absent, and the group's skips and ML bytes
 * are skips[off[g] .. off[g + 1]) and ml[off[g] .. off[g + 1]).  Positions are those of the read as the set holds it (an nt16 record added with
 * reverse != 0 is turned back by the set, so MM needs no turning).  The arrays are copied.  MM_ERR_ARG: no sequence yet, a second call for one
 * sequence, a set that is uploaded, n_groups outside [0, 255], a base outside ACGT, a code outside [-1, 3], a mode other than the three, offsets
 * that start below 0 or fall, a null array.  mm_seqset_upload writes the plane with one wavefront per read: who (0 no call, 1 canonical, 2 another
 * code, 3 + code) and prob per base.  A group that names more occurrences of its base than the sequence has is MM_ERR_DATA, mm_last_error names the
 * lowest such sequence and its lowest such group.  A set without any mm_seqset_add_mods call allocates and launches nothing for modifications.
 * mm_seqset_has_mods: 1 if any sequence of the set got a call.  mm_seqset_fetch_mods: who and prob of sequence i in read order (cap >= its length),
 * zeros for a sequence without groups.  mm_seqset_slice and mm_seqset_concat carry the plane (a part without one gives zeros); mm_seqset_save / _load
 * and mm_seqset_hpc do not. */
int mm_seqset_add_mods(mm_seqset* s, int32_t n_groups, const uint8_t* base, const int8_t* code /* -1..3 */, const uint8_t* mode,
                       const int64_t* off /* [n_groups + 1] */, const uint32_t* skips, const uint8_t* ml);
int mm_seqset_has_mods(const mm_seqset* s);
int mm_seqset_fetch_mods(mm_seqset* s, int64_t i, uint8_t* who_out, uint8_t* prob_out, int64_t cap);
/* Inflate n BGZF blocks (whole gzip members with the BC field: header + deflate + CRC32 + ISIZE) on the context's device, from host memory
 * into host memory.  Block i is comp[comp_off[i], comp_off[i] + comp_len[i]) (comp_bytes bytes in `comp`); its ISIZE inflated bytes go to
 * out[out_off[i], out_off[i] + ISIZE) (out_cap bytes in `out`); no other byte of `out` is written, nor the bytes of a block that fails.
 * status[i] (may be NULL): 0 ok, 1 deflate stream invalid, 2 length != ISIZE (or ISIZE > 65536), 3 CRC32 mismatch, 4 malformed gzip
 * header (shorter than 26 bytes, or the extra field runs into the trailer).  Returns MM_OK if every block is ok, MM_ERR_ARG for bad
 * arguments (a block outside `comp`, or a readable ISIZE that does not fit `out` at its offset), MM_ERR_DATA if any block is bad. */
int mm_bgzf_inflate(mm_ctx* ctx, const uint8_t* comp, int64_t comp_bytes, const int64_t* comp_off, const int32_t* comp_len, int32_t n,
                    uint8_t* out, int64_t out_cap, const int64_t* out_off, int32_t* status);
/* Deflate in_bytes bytes of host memory into BGZF on the context's device: the input is cut into blocks of 65 280 bytes and each becomes one
 * complete BGZF member (header with the BC subfield and BSIZE, one DEFLATE block with dynamic Huffman codes — stored where that would not be
 * smaller —, CRC32, ISIZE; LZ77 over a 32 KiB window inside the block).  The members go back to back into out[0, *out_bytes); *n_blocks is
 * their number.  The bytes are a function of the input alone (not of the device, the grid or the call that carries a block).  in_bytes == 0
 * gives zero blocks and *out_bytes == 0.  The 28-byte BGZF end-of-file block is NOT appended: the caller writes it once when it closes the
 * file.  MM_ERR_ARG for a null pointer or an out_cap below mm_bgzf_deflate_bound(in_bytes).  With MM_DEFLATE_HOST=1 in the environment the
 * same container is written by zlib level 1 on the host's threads (other bytes, the same inflated text). */
int64_t mm_bgzf_deflate_bound(int64_t in_bytes);   /* bytes `out` must hold for any input of that size */
int mm_bgzf_deflate(mm_ctx* ctx, const uint8_t* in, int64_t in_bytes, uint8_t* out, int64_t out_cap, int64_t* out_bytes, int32_t* n_blocks);
/* Plain gzip (RFC 1952: any number of members, each one DEFLATE stream without a block index) inflated on the context's device, from host
 * memory into host memory, a segment at a time ("Plain gzip on the device").  The compressed stream is cut into chunks of
 * chunk_bytes (0: MM_GZIP_CHUNK_BYTES, else 256 KiB) and each chunk decoded speculatively from a block start it finds, then checked against its
 * predecessor; segment_bytes (0: 128 MiB, at most 1 GiB) is how much compressed input one round takes.  Device memory of a stream: the round's
 * chunk slots, kept within 4.5 GiB (a small chunk_bytes shortens the round instead), two segments of input and a round's output.
 *   mm_gzip_open   a stream on ctx (ctx outlives it; the one-thread-per-context rule holds for the stream's calls too)
 *   mm_gzip_feed   the next n compressed bytes (all are taken; last != 0: they end the file).  *avail (may be NULL): inflated bytes ready to
 *                  read.  Output is produced once a segment's worth of input is buffered, and at the end.  Header fields (FEXTRA, FNAME,
 *                  FCOMMENT, FHCRC) are parsed, concatenated members read through, each member's CRC32 and ISIZE checked, and bytes behind a
 *                  member that do not start a gzip header are ignored (as zlib's gzread ignores them).  MM_ERR_DATA for a corrupt or
 *                  truncated stream: mm_last_error names the compressed byte offset, and every later feed fails the same way.
 *   mm_gzip_read   up to cap inflated bytes into out, *got of them
 *   mm_gzip_stats  counts[5]: chunks, chunks whose speculation was accepted, chunks decoded again from their predecessor's end, chunks covered
 *                  by their predecessor's decode (no block starts in them), members; seconds[4]: speculative kernel, sequential walk (with the
 *                  decodes again), resolve + CRC, all of feed.  Either pointer may be NULL.
 *   mm_gzip_close  frees the stream */
int mm_gzip_open(mm_ctx* ctx, int64_t chunk_bytes, int64_t segment_bytes, mm_gzip** out);
int mm_gzip_feed(mm_gzip* g, const uint8_t* comp, int64_t n, int last, int64_t* avail);
int mm_gzip_read(mm_gzip* g, uint8_t* out, int64_t cap, int64_t* got);
int mm_gzip_stats(const mm_gzip* g, int64_t* counts, double* seconds);
void mm_gzip_close(mm_gzip* g);
int mm_seqset_upload(mm_seqset* s);                                /* pack + copy to HBM; set is then frozen.  Packs into the CONTEXT's pinned
                                                                    * staging buffer: two uploads of sets of one context must not overlap (the one-thread-
                                                                    * per-context rule above applies to this entry point too) */
/* Persistent packed form of an uploaded sequence set (2-bit bases, exception runs, lengths): what `metamaps index` stores
 * per index chunk in place of the reference's Boost archive of the sketch (createIndex, mapWrap.h:358-405;
 * winSketch.hpp:73-83).  The device index is rebuilt from it in seconds (mm_index_build), nothing derived is stored. */
int mm_seqset_save(mm_seqset* set, const char* path);
int mm_seqset_load(mm_ctx* ctx, const char* path, mm_seqset** out);
/* Sequences [first, first + count) of an uploaded set as a set of their own, and several uploaded sets of one device back to back
 * as one — device-side copies of the packed stream, nothing is packed again.  The CLI uploads the reference in bounded groups as
 * its parser delivers the contigs (the reference streams contig by contig, winSketch.hpp:242-252), concatenates them and cuts
 * the index chunks of --maxmemory (winSketch.hpp:274-329) out of the resident whole. */
int mm_seqset_slice(mm_ctx* ctx, const mm_seqset* set, int64_t first, int64_t count, mm_seqset** out);
int mm_seqset_concat(mm_ctx* ctx, const mm_seqset* const* parts, int n_parts, mm_seqset** out);
int64_t mm_seqset_count(const mm_seqset* s);
int64_t mm_seqset_total_bases(const mm_seqset* s);
int mm_seqset_lengths(const mm_seqset* s, int32_t* len_out /* [count] */);
/* read back sequence i as (upper-cased) ASCII — round-trip check for tests */
int mm_seqset_fetch(mm_seqset* s, int64_t i, char* ascii_out, int64_t cap);
/* sequences [first, first + count) one behind the other, no separators (lengths: mm_seqset_lengths); cap >= their total length */
int mm_seqset_fetch_range(mm_seqset* s, int64_t first, int64_t count, char* ascii_out, int64_t cap);

/* Homopolymer compression (mapDirectly --hpc; not in the reference).  hpc(S) replaces every maximal run of equal bytes
 * of S — as the pipeline hashes it: upper-cased ASCII, IUPAC and N bytes kept — by one such byte ("NNNN" -> "N", "aAaA" -> "A", "NNRRNN" ->
 * "NRN", empty stays empty).  mm_seqset_hpc compresses every sequence of an uploaded set on the device into a new set in the same layout
 * (`raw` is left as it is and may be destroyed): every other entry point takes the result as it takes an uploaded set.  `map` (NULL: not
 * wanted, e.g. for reads) receives the coordinate map back to raw positions, 0.133 bytes per raw base on the device:
 *   raw(i, p)      0 <= p < clen: the raw position of the first base of the run that became base p of sequence i; p >= clen: rawlen + (p - clen)
 *                  (the reference reports end = start + len - 1 without clamping, so positions past the end translate too); p < 0: p
 *   rawlast(i, p)  the raw position of the last base of that run, the same rule beyond the end
 * mm_hpc_map_to_raw evaluates both for n (sequence, compressed position) pairs given in host arrays (either output may not be NULL).
 * mm_mapping_to_raw rewrites the records of `m` on the device, after mm_mapping_add_qualities: ref_start becomes raw(ref_contig, ref_start),
 * and end_out[i] (host, cap >= number of records) receives rawlast(ref_contig, ref_start + read length - 1) of record i, with the lengths
 * the mapping was made with (the compressed reads').  ref_contig indexes the set `ref_map` was made from: call it on the merged mapping
 * (mm_mapping_concat / _gather / _from_parts), whose contig ids are those of the whole reference.  Call it once per mapping. */
int mm_seqset_hpc(mm_ctx* ctx, const mm_seqset* raw, mm_seqset** out, mm_hpc_map** map);
int mm_hpc_map_to_raw(mm_hpc_map* map, const int32_t* seq, const int64_t* pos, int64_t n, int64_t* first_out, int64_t* last_out);
int mm_hpc_map_lengths(const mm_hpc_map* map, int32_t* raw_len /* [count], may be NULL */, int32_t* compressed_len /* [count], may be NULL */);
int64_t mm_hpc_map_device_bytes(const mm_hpc_map* map);
int mm_mapping_to_raw(mm_ctx* ctx, mm_mapping* m, const mm_hpc_map* ref_map, int64_t* end_out, int64_t cap);
void mm_hpc_map_destroy(mm_hpc_map* map);

/* Device-side synthetic inputs (bench.py; DESIGN.md "Synthetic workload").  The reference is a set of
 * genomes grouped in species (strains = substituted copies of a species root), generated straight into
 * packed HBM form; reads are sampled from it with ONT/PacBio-like sub/ins/del errors. */
typedef struct {
  uint64_t seed;
  int32_t n_species;          /* species roots                                                     */
  int32_t strains_per_species;
  int32_t genome_len;         /* bases per genome (one contig per genome)                          */
  float strain_divergence;    /* per-base substitution rate of a strain w.r.t. its species root    */
  float genus_divergence;     /* roots of the same genus (4 species each) differ by this rate      */
} mm_synth_ref_params;
typedef struct {
  uint64_t seed;
  int64_t n_reads;
  int32_t read_len;           /* template length taken from the genome                              */
  float sub_rate, ins_rate, del_rate;
  float frac_random;          /* reads made of random sequence (unmappable)                          */
  int32_t n_abundant;         /* reads are drawn from this many genomes, lognormal abundances        */
  int32_t read_len_min;       /* 0: every read has read_len bases; else lengths log-uniform in [read_len_min, read_len] */
} mm_synth_read_params;
int mm_synth_reference(mm_ctx* ctx, const mm_synth_ref_params* p, mm_seqset** out);
/* The miniSeq+H-shaped community of SURVEY.md §8 D1: microbial genomes of lognormal length grouped in species of 1..12 strains
 * (substitutions at a per-strain rate + a few block insertions / deletions against the species root), species roots grouped in
 * genera; plus "human-like" contigs: `repeat_fraction` of their 256-base granules are copies (2-20 % diverged, either strand) of
 * granules of a Zipf-weighted repeat family library, and `n_fraction` of their bases are runs of N.  Contig order is shuffled.
 * contig_genome[n_contigs] (optional) receives the genome of every contig: 0 .. n_genomes-1 microbial (one contig each), n_genomes
 * for every human-like contig.  n_contigs = n_genomes + human_contigs. */
typedef struct {
  uint64_t seed;
  int32_t n_genomes, n_species, n_genera;      /* microbial genomes (= contigs), species (1..12 strains each), genera        */
  double median_len, sigma_len;                /* lognormal genome length, clipped to [min_len, max_len]                    */
  int32_t min_len, max_len;
  float strain_div_min, strain_div_max;        /* substitution rate of a strain against its species root                    */
  float genus_div_min, genus_div_max;          /* substitution rate of a species root against its genus root                */
  int32_t strain_indel_events;                 /* up to this many block insertions / deletions (50 - 5000 bases) per strain  */
  int32_t human_contigs;                       /* 0: none                                                                    */
  int64_t human_bases;                         /* total length of the human-like contigs                                     */
  float repeat_fraction, n_fraction;
  int32_t n_repeat_families;
  int64_t total_bases_target;                  /* > 0: microbial lengths are scaled so that everything sums to this          */
} mm_synth_community_params;
int mm_synth_community(mm_ctx* ctx, const mm_synth_community_params* p, mm_seqset** out, int32_t* contig_genome);
/* genome_species[n_genomes]: the species (0 .. n_species-1) of every microbial genome of the community the same parameters generate
 * (host arithmetic only: the truth labels of bench.py's and the full-size tests' species-level checks) */
int mm_synth_community_species(const mm_synth_community_params* p, int32_t* genome_species);
/* truth_genome (optional, [n_reads]) receives the source contig index or -1.  Reads are drawn from `n_abundant` contigs among
 * those long enough for the longest read (exception runs — N — of the reference read as A). */
int mm_synth_reads(mm_ctx* ctx, const mm_seqset* reference, const mm_synth_read_params* p, mm_seqset** out,
                   int32_t* truth_genome);

/* ---- A2 debug tap: winnowed minimizers of every sequence (commonFunc.hpp:92-175) -------------- */
/* offsets[count+1]; records are (hash, wpos, strand) in winnowing order.  Pass NULL arrays to query sizes. */
int mm_minimizers(mm_ctx* ctx, const mm_seqset* s, int k, int w, int64_t* offsets, uint32_t* hash, int32_t* wpos,
                  int32_t* strand, int64_t cap);

/* ---- index (replaces Sketch::build_and_store_index + computeFreqHist, winSketch.hpp:180-365, :452-494) */
typedef struct {
  int64_t n_contigs, n_entries, n_unique_hashes, n_dup_flagged;
  int64_t hbm_bytes;
} mm_index_info;
int mm_index_build(mm_ctx* ctx, const mm_seqset* contigs, int k, int w, mm_index** out);
void mm_index_destroy(mm_index* idx);
/* Persistent device index: what createIndex stores and mapAgainstIndex loads per index chunk (written mapWrap.h:388-391, read :525-529;
 * the Boost archives of winSketch.hpp:73-83), in an own versioned binary format — the index arrays as they lie in HBM (entries, occurrence
 * lists + bins, hash table, position directory, duplicate distances), the contig lengths, the occurrence histogram of the chunk (so that
 * the accumulated freqThreshold of winSketch.hpp:452-494 comes out as after a build) and the threshold that was set when it was stored.
 * A load is file -> pinned staging -> device, no kernel runs; the loaded index behaves as the built one in every entry point.
 * MM_ERR_ARG with a message for an unreadable, foreign, truncated or inconsistent file. */
int mm_index_save(mm_index* idx, const char* path);
int mm_index_load(mm_ctx* ctx, const char* path, mm_index** out);
/* --maxmemory chunk rule (Sketch::build flush test winSketch.hpp:274-329, memory model :165-178), evaluated on the
 * index of the WHOLE reference: returns the first contig of every chunk the reference would create under the
 * given limit (n_chunks == 1, first_contig[0] == 0 when everything fits or max_memory_bytes == 0).  The caller then
 * builds one mm_index per contig range, maps every read against each, and merges with mm_mapping_concat.
 * MM_ERR_LIMIT if a single contig exceeds the limit (the reference throws there, :318-322). */
int mm_index_plan_chunks(mm_ctx* ctx, const mm_index* whole, uint64_t max_memory_bytes, int32_t* first_contig, int32_t cap, int32_t* n_chunks);
int mm_index_get_info(const mm_index* idx, mm_index_info* out);
/* Occurrence-count histogram of this chunk: pairs (count, number of hashes with that count), ascending.
 * The caller accumulates it across chunks and derives freqThreshold exactly as winSketch.hpp:452-494 does
 * (mm_freq_threshold_from_hist below) — the reference never clears the histogram between chunks. */
int mm_index_freq_hist(mm_index* idx, int64_t* counts, int64_t* n_hashes, int64_t cap, int64_t* n_out);
int mm_freq_threshold_from_hist(const int64_t* counts, const int64_t* n_hashes, int64_t n, int64_t n_unique_hashes,
                                int prev_threshold);
int mm_index_set_freq_threshold(mm_index* idx, int threshold);
/* debug tap: position-ordered entries (hash, contig, wpos, strand) */
int mm_index_entries(mm_index* idx, uint32_t* hash, int32_t* contig, int32_t* wpos, int32_t* strand, int64_t cap);
/* debug tap: per entry, the distance in entries to the previous / next entry of its contig with the same hash (0: there is none),
 * saturated at 65535 — what K5 answers slidingMap.hpp:139-214's "is this hash already / still inside the window?" from */
int mm_index_dup_neighbours(mm_index* idx, int32_t* prev_dist, int32_t* next_dist, int64_t cap);

/* ---- host statistics (float math of map_stats.hpp; Boost.Math binomial restated) -------------- */
int mm_recommended_window(double p_value, int k, float pi, int min_read_len, uint64_t reference_size);   /* map_stats.hpp:226 */
double mm_estimate_pvalue(int s, int k, float pi, int min_read_len, uint64_t reference_size);             /* map_stats.hpp:179 */
int mm_min_hits_relaxed(int s, int k, float pi);                                                          /* map_stats.hpp:142 */
void mm_identity(int shared, int s, int k, float* ident, float* ident_upper /* may be NULL */);         /* computeMap.hpp:406-412 */

/* ---- mapping (replaces Map::mapModule for a whole batch: computeMap.hpp:180-538) -------------- */
typedef struct {
  int32_t k, w;
  float perc_identity;        /* --pi, default 80                                   */
  int32_t min_read_len;       /* reads shorter than max(w,k,min_read_len) are skipped (computeMap.hpp:137) */
} mm_map_params;

typedef struct {              /* one L2 mapping that passed the identity filter (base_types.hpp:133) */
  int32_t read;               /* index of the read in the seqset                      */
  int32_t ref_contig;         /* chunk-local contig id                                */
  int32_t ref_start;          /* meanOptimalPos; refEnd = ref_start + read_len - 1    */
  int32_t shared;             /* conservedSketches                                    */
  int32_t sketch;             /* sketchSize s                                         */
  int32_t strand;             /* +1 / -1                                              */
  double mapq;                /* mapping quality (mapWrap.h:215-323), filled by mm_mapping_add_qualities */
} mm_map_record;

typedef struct {
  int64_t n_reads, n_reads_long_enough, n_reads_mapped, n_mappings;
  int64_t bases_long_enough;
  /* algorithmic-traffic counters */
  int64_t sum_sketch, sum_hits, n_candidates, sum_l2_stream_entries, sum_l2_evals;
  int64_t n_ambiguous_sketch_reads;   /* reads whose duplicate-hash strands needed the std::sort tie-break */
  int64_t sum_hits_kept;              /* seed hits left after the exact run pre-filter (K3c) */
  int64_t n_l2_rebuilds;              /* window states rebuilt from scratch by the exact skip-ahead of K5 */
  int64_t n_l2_wide_redo;             /* candidates done again: by the literal full slide (reads shorter than w+k) or after a strand tie-break */
  /* device time of each stage of this batch, milliseconds, from hipEvents recorded on the ctx stream
   * around the launches; ms_l2 (the K5/K6 kernel) and ms_hit_filter (the counting+filtering K3c kernel, part of
   * ms_probe_gather) are single kernels: bench.py's roofline uses whichever is larger */
  double ms_minimizer, ms_sketch, ms_probe_gather, ms_sort_hits, ms_l1_scan, ms_l2, ms_compact, ms_total, ms_hit_filter;
  /* reads whose sketch has >= 32768 hashes (longer than ~145 kb at w = 8): mapped like every other read, but by the slow
   * K5 class that keeps its window state in global memory (informational) */
  int64_t n_reads_giant;
} mm_map_stats;

int mm_map_batch(mm_ctx* ctx, const mm_index* idx, const mm_seqset* reads, const mm_map_params* p, mm_mapping** out);
/* mm_map_batch with two stage boundaries handed to the caller: `at_stage(user, stage)` is called on the calling thread, at most once per
 * stage and not at all when the batch fails or ends before that point:
 *   stage 1  the sketches of the batch are complete (K1 + K2 have run), nothing of its seed stage (K3) is enqueued yet;
 *   stage 2  the last big kernel of the batch (K5 / K6) is enqueued; what follows are small kernels and downloads.
 * A caller that drives several contexts of one device decides with it which stages of two batches may share the GPU: bench.py lets
 * the next batch start at stage 2 (its minimizer stage takes the CUs that this batch's last kernel leaves as it drains), or — with
 * --staged-map — takes one lock for K1 + K2 and another for K3 ... K6 and swaps them at stage 1.  The callback must not call into
 * `ctx`; results are the same with or without it. */
int mm_map_batch_phased(mm_ctx* ctx, const mm_index* idx, const mm_seqset* reads, const mm_map_params* p, void (*at_stage)(void* user, int stage), void* user,
                        mm_mapping** out);
/* The same batch against another index (the next chunk of --maxmemory): minimizers and sketches of the reads — which do not depend on
 * the index — are taken from `sketch_of` (the two large read-only arrays held jointly when it belongs to `ctx`, everything copied otherwise), a mapping of THESE reads with the same k, w and minimum read length whose intermediates
 * have not been released, instead of being computed again (the reference recomputes them per chunk, computeMap.hpp:277-298).
 * Results are those of mm_map_batch. */
int mm_map_batch_reusing(mm_ctx* ctx, const mm_index* idx, const mm_seqset* reads, const mm_map_params* p, const mm_mapping* sketch_of, mm_mapping** out);
/* Minimizers and sketches of a read batch alone (K1 + K2, computeMap.hpp:277-298) — a `sketch_of` for mm_map_batch_reusing that is tied to
 * no index: a run that maps one batch against many chunk indexes one after the other, each built and dropped in turn, computes them once
 * and keeps nothing else of a chunk's mapping.  The object holds no records (the other mm_mapping_* calls see an empty mapping);
 * mm_mapping_destroy frees it. */
int mm_sketch_batch(mm_ctx* ctx, const mm_seqset* reads, const mm_map_params* p, mm_mapping** out);
void mm_mapping_destroy(mm_mapping* m);
int mm_mapping_get_stats(const mm_mapping* m, mm_map_stats* out);
/* frees everything of a batch result but its records, offsets and read lengths (what fetch, keep_best, concat, add_qualities and
 * the EM builder use); the debug taps return empty afterwards.  For callers that hold the results of many batches, e.g. while
 * the chunks of a reference larger than HBM are indexed and mapped one after the other (mapWrap.h:417-437 keeps them as files). */
int mm_mapping_release_intermediates(mm_mapping* m);
/* per-read first-record offsets [n_reads+1], records in (read, contig, position) order */
int mm_mapping_fetch(mm_mapping* m, int64_t* offsets, mm_map_record* records, int64_t cap);
/* K8: mapping qualities over the union of each read's records (mapWrap.h:215-323) */
int mm_mapping_add_qualities(mm_ctx* ctx, mm_mapping* m, const mm_seqset* reads, int k);
/* default (non --all) reporting: per read keep the records whose identity is >= best - 1.0
 * (reportReadMappings, computeMap.hpp:546-587).  Apply per index chunk, before mm_mapping_concat / add_qualities. */
int mm_mapping_keep_best(mm_ctx* ctx, mm_mapping* m, int k);
/* merge the records of several index chunks read-wise, chunk order preserved (unifyFiles, mapWrap.h:128-132), on the device.  The parts may
 * belong to any context of this process: records of a part on another device are fetched with a peer copy.  The result carries
 * records only (as after mm_mapping_release_intermediates: the debug taps return MM_ERR_STATE); its statistics are the work
 * counters and stage times summed over the parts. */
int mm_mapping_concat(mm_ctx* ctx, mm_mapping* const* parts, const int32_t* contig_base, int n_parts, mm_mapping** out);
/* the same from host-side parts, i.e. what mm_mapping_fetch returned for index chunks that live on OTHER GPUs (SURVEY §8 E1:
 * "records gathered to the read's owner"; the reference gathers them through its PREFIX.N files, mapWrap.h:417-437):
 * offsets[p][n_reads+1] and records[p][...] of chunk p, contig_base[p] = first contig of chunk p in the whole reference.
 * The result carries records only (as after mm_mapping_release_intermediates) and takes mm_mapping_add_qualities,
 * mm_mapping_fetch and mm_em_create_from_mapping. */
int mm_mapping_from_parts(mm_ctx* ctx, int64_t n_reads, const int32_t* read_len, const mm_map_params* p, int n_parts,
                          const int64_t* const* offsets, const mm_map_record* const* records, const int32_t* contig_base, mm_mapping** out);

/* the same exchange between the RANKS of ctx's communicator (mm_comm_init; one process per GPU, or one host thread per GPU of one process), device
 * to device over RCCL (ncclSend / ncclRecv over xGMI) — nothing is staged in host memory.  Collective: every rank calls it for the
 * same read batch, batches in the same order on every rank.  parts[i] = this rank's mapping of the batch against chunk chunk_id[i] (it must hold
 * every chunk c with chunk_rank[c] == its rank); n_chunks / chunk_rank[c] / contig_base[c] describe all chunks of the reference and are the same
 * on every rank.  On rank `owner`, *out receives the merged mapping (records only, chunk order; takes mm_mapping_add_qualities ...); on the other
 * ranks *out = NULL.  A one-rank communicator (or none) merges locally. */
int mm_mapping_gather(mm_ctx* ctx, int owner, int64_t n_reads, const int32_t* read_len, const mm_map_params* p, mm_mapping* const* parts, const int32_t* chunk_id,
                      int n_parts, int n_chunks, const int32_t* chunk_rank, const int32_t* contig_base, mm_mapping** out);

/* debug taps for one batch (parity tests).  Any output pointer may be NULL. */
int mm_debug_sketch(mm_mapping* m, int64_t* offsets, uint32_t* hash, int32_t* strand, int64_t cap);          /* computeMap.hpp:292-298 */
int mm_debug_hits(mm_mapping* m, int64_t* offsets, int32_t* contig, int32_t* wpos, int64_t cap);             /* :307-323, sorted :353 */
int mm_debug_candidates(mm_mapping* m, int64_t* offsets, int32_t* triples /* contig,start,end */, int64_t cap);   /* :346-386 */
int mm_debug_l2(mm_mapping* m, int64_t* per_cand /* contig, meanPos, shared, optBeg, optEnd, accepted */, int64_t cap);      /* :460-538 */
int mm_debug_min_hits(mm_mapping* m, int32_t* min_hits /* [n_reads] */);
/* measurement tap: lengths of the occurrence lists the batch's sketch hashes ask `idx` for (minimizerPosLookupIndex.find, computeMap.hpp:310):
 * hist[0] = hashes not in the index, hist[c] = lists of c entries (c < n_bins - 2), hist[n_bins - 2] = longer lists that are kept,
 * hist[n_bins - 1] = lists cut by freqThreshold (:317) */
int mm_debug_probed_lists(mm_mapping* m, const mm_index* idx, int64_t* hist, int32_t n_bins);

/* ---- EM (replaces meta::doEM's iteration, fEM.h:501-661, and the per-read likelihood fEM.h:234-373) */
/* Mappings are given read-wise: read r owns entries [read_off[r], read_off[r+1]).  For entry i:
 * l_i = f[taxon[i]] * inv_nloc[i] * mapq[i]  (fEM.h:353), p_i = l_i / sum over the read.  */
int mm_em_create(mm_ctx* ctx, int64_t n_reads, const int64_t* read_off, const int32_t* taxon, const double* mapq,
                 const double* inv_nloc, int32_t n_taxa, mm_em** out);
/* map -> classify without the text file in between: the same EM problem `classify` would read from PREFIX, built on
 * the device from the records of `m` (after mm_mapping_add_qualities): taxon = contig_taxon[contig]; the mapping
 * quality rounded to the 6 significant digits the file carries (mapWrap.h:318-320 -> fEM.h:262); 1/nLoc with
 * nLoc = sum over the taxon's contigs of (len - readLen + 1) when len >= readLen, else 1 if the read maps to that
 * contig (getMappingLocations, fEM.h:322-346). */
int mm_em_create_from_mapping(mm_ctx* ctx, const mm_mapping* m, const int32_t* contig_taxon, const int32_t* contig_len, int32_t n_contigs,
                              int32_t n_taxa, mm_em** out);
/* mappings per taxon (taxa without any start the iteration at frequency 0, fEM.h:494) */
int mm_em_taxon_counts(mm_em* em, int64_t* counts);
int mm_em_sizes(const mm_em* em, int64_t* n_reads, int64_t* n_entries, int32_t* n_taxa);
void mm_em_destroy(mm_em* em);
/* one E+M step on this rank's reads: f_partial[t] = sum of p_i, *ll_partial = sum log(sum l_i) */
int mm_em_iterate(mm_em* em, const double* f, double* f_partial, double* ll_partial);
/* same, but leaves the partial sums on the device, all-reduces them over the communicator (RCCL) and
 * returns the normalised next f and the global log-likelihood (identical on every rank) */
int mm_em_iterate_allreduce(mm_em* em, const double* f, double* f_next, double* ll);
/* The whole loop of meta::doEM (fEM.h:501-661) without a host round trip per iteration: starting from f0, iterate (E step, per-taxon
 * sums, all-reduce over the communicator if there is one, normalise) until the reference's stop rule fires (log-likelihood gain <= 1
 * and relative gain < 1e-4, from the second iteration on) or max_iter iterations.  f_out[n_taxa] = final frequencies, ll_trace
 * (optional, up to ll_cap <= 1024 values) = log-likelihood of every iteration, *n_iter = iterations done.  Every rank of the
 * communicator calls it together and gets the same result. */
int mm_em_run(mm_em* em, const double* f0, int max_iter, double* f_out, double* ll_trace, int ll_cap, int* n_iter);
/* Goes on where the previous mm_em_run / mm_em_continue on `em` ended (same f, iteration count, previous log-likelihood) for up to
 * max_iter more iterations; ll_trace receives the log-likelihoods of THESE iterations, *n_iter their number, *stopped (optional)
 * whether the stop rule has fired (then further calls do nothing).  A caller that wants every round's log-likelihood of a long
 * run (the reference prints each, fEM.h:616-634) calls mm_em_run and then mm_em_continue in slices of <= 1024 iterations. */
int mm_em_continue(mm_em* em, int max_iter, double* f_out, double* ll_trace, int ll_cap, int* n_iter, int* stopped);
/* final posteriors p_i for the current f (fEM.h:684-707) and the index of the best mapping per read (fEM.h:217) */
int mm_em_posteriors(mm_em* em, const double* f, double* post /* [n_entries] */, int64_t* best /* [n_reads] */);
/* Read-level Poisson bootstrap of the EM (not in the reference): replicates rep0 .. rep0+n_rep-1 of `em`, each the weighted EM
 * started from f_start with weights w(r,i) = boot_weight(seed, r, i), or weights[(r-rep0)*n_reads + i] if weights != NULL.
 * f_out [n_rep*n_taxa] (replicate-major), ll_out [n_rep], n_iter [n_rep], stopped [n_rep] (1: stop rule, 0: max_iter reached).
 * Read i is the i-th read WITH a mapping (reads without one are not resampled), so n_reads above counts those reads.  The stop rule is
 * mm_em_run's, per replicate; a replicate that has stopped is frozen.  A replicate whose weighted sample is EMPTY (no read with a mapping
 * has a weight > 0, or `em` has no mapping at all) has no estimate: its f_out row is all 0, ll_out 0, n_iter 0, stopped 1, and it costs no
 * iterations.  max_iter <= 0 is refused, so n_iter == 0 identifies such a replicate: a caller leaves it out of its statistics (the chance
 * is e^-n per replicate for n reads with a mapping).  The other replicates are what they are without it.  Results do not depend on how
 * the replicates are split over calls or devices.  The communicator of the context is never used.  MM_ERR_LIMIT when the per-replicate buffers (n_entries*n_rep*8 bytes of
 * posteriors and n_taxa*n_rep*8 of frequencies) exceed the device, MM_ERR_NOMEM when they do not fit its free memory: the caller tiles. */
int mm_em_bootstrap(mm_em* em, const double* f_start, int32_t rep0, int32_t n_rep, uint64_t seed, const uint8_t* weights,
                    int max_iter, double* f_out, double* ll_out, int32_t* n_iter, int32_t* stopped);
/* Confidence-thresholded lowest-common-ancestor assignment of every read of `em` (not in the reference).
 * Tree: n_nodes nodes, parent[v] < v for v > 0, parent[0] == 0 (the root); taxon_node[n_taxa]: the node of every taxon of `em`.
 * Posteriors are those of mm_em_posteriors(em, f).  node_out[n_reads]: lca(r), or -1 for a read without entries; mass_out[n_reads]
 * (may be NULL): mass(r, lca(r)), 0 for such a read; direct_out[n_nodes] (may be NULL): reads per assigned node.
 * MM_ERR_ARG: threshold outside [0.51, 1], a parent[] that is not in that order, a taxon_node outside the tree. */
int mm_em_lca(mm_em* em, const double* f, int32_t n_nodes, const int32_t* parent, const int32_t* taxon_node, double threshold,
              int32_t* node_out, double* mass_out, int64_t* direct_out);

/* ---- gene-level analysis (classify --genes; the reference's geneLevelAnalysis.pl) ---------------------- */
/* Which annotated genes do mappings overlap.  Genes: those of contig c are [contig_gene_off[c], contig_gene_off[c+1]), sorted by Start within
 * the contig, Start and Stop inclusive; gene_group[j] in [0, n_groups): genes of one group are pooled.  group_feat_off[n_groups+1] /
 * group_feat: the feature ids (in [0, n_feats)) a group's protein carries.  Mapping (c, s, e) overlaps gene (Start, Stop) of contig c iff
 * Start < e && s <= Stop.  group_reads[g]: overlaps of the group's genes (a mapping that overlaps two of them counts twice);
 * group_median[g]: the element of 0-based rank (n-1)/2 of the identities of those overlaps in ascending order, NaN where group_reads is 0;
 * feat_reads[f] (may be NULL): mappings that overlap at least one gene whose group carries f; maps_on_annotated (may be NULL): mappings on
 * contigs with at least one gene.  Zero genes or zero mappings are valid.  MM_ERR_ARG: offsets that do not start at 0 and ascend, genes not
 * sorted by Start within a contig, Stop < Start, a gene_group, feature id or map_contig out of range, map_stop < map_start, a negative or
 * NaN identity.  MM_ERR_LIMIT: 2^32 mappings or more.  The device buffers are tiled to MM_GENE_PAIR_BUDGET pairs; no result depends on it. */
int mm_gene_overlap(mm_ctx* ctx, int32_t n_contigs, const int64_t* contig_gene_off, const int32_t* gene_start, const int32_t* gene_stop,
                    const int32_t* gene_group, int32_t n_groups,
                    const int64_t* group_feat_off /* [n_groups+1] */, const int32_t* group_feat, int32_t n_feats,
                    int64_t n_maps, const int32_t* map_contig, const int32_t* map_start, const int32_t* map_stop, const double* map_ident,
                    int64_t* group_reads /* [n_groups] */, double* group_median /* [n_groups], NaN where group_reads is 0 */,
                    int64_t* feat_reads /* [n_feats], may be NULL */, int64_t* maps_on_annotated /* may be NULL */);

/* ---- identity filter (classify --min-identity; the reference's util/filterLowIdentityEntities.pl) ------------ */
/* Which genomes of an EM problem have best mappings of low median identity, and the EM problem without them.  Reads r with entries
 * [read_off[r], read_off[r+1]); taxon[i] in [0, n_taxa); ident[i]: the entry's identity in percent; best[r]: an entry of read r (ignored for a
 * read without entries).  sorted_max: the largest identity of every read with entries, ascending (room for n_reads values; n_with_entries are
 * written); n_le: how many of them are <= thr_percent.  taxon_reads[t]: reads with taxon[best[r]] == t; taxon_median[t]: the element of 0-based
 * rank taxon_reads[t] / 2 of their ident[best[r]] in ascending order (the upper median), NaN where there is none; taxon_removed[t] =
 * taxon_reads[t] > 0 && taxon_median[t] < thr_percent; read_removed[r] = taxon_removed[taxon[best[r]]], 0 for a read without entries.
 * The filtered problem (all five NULL, or none): an entry is kept iff its taxon is not removed, a read iff it keeps an entry; entry_src
 * (room for all entries) and read_src (room for n_reads) are the original indices of the kept ones, ascending; read_off_out (room for
 * n_reads + 1) the offsets of the kept reads into entry_src.  Zero reads and zero entries are valid.  Nothing is written on an error.
 * MM_ERR_ARG: offsets that do not start at 0 and ascend, a taxon out of range, a best[r] outside its read's entries, a negative or NaN identity
 * (-0.0 is taken as 0), a NaN threshold.  MM_ERR_LIMIT: 2^32 reads or more (ranks are 32-bit; entry indices are 64-bit). */
int mm_ident_filter(mm_ctx* ctx, int64_t n_reads, const int64_t* read_off /* [n_reads+1] */, const int32_t* taxon, const double* ident,
                    const int64_t* best /* [n_reads] */, int32_t n_taxa, double thr_percent,
                    double* sorted_max /* [reads with entries] */, int64_t* n_with_entries, int64_t* n_le,
                    int64_t* taxon_reads /* [n_taxa] */, double* taxon_median /* [n_taxa] */, uint8_t* taxon_removed /* [n_taxa] */,
                    uint8_t* read_removed /* [n_reads] */,
                    int64_t* read_src, int64_t* entry_src, int64_t* read_off_out, int64_t* n_reads_out, int64_t* n_entries_out);

/* Exact edit distances (not in the reference; DESIGN.md section 1, "Edit distances"; the definition: csrc/mm_edit_core.hpp), by Myers' bit-vector
 * recurrence on the device, one job per wavefront.  Job i aligns read read[i] of `reads` (its reverse complement for strand[i] == -1, the whole
 * read) to the window [ws[i], we[i]) of contig contig[i] of `reference`, the window's ends free: dist_out[i] is the smallest unit-cost Levenshtein
 * distance d to a substring of the window, end_out[i] the smallest end b (window coordinates, half-open) of a substring at that distance,
 * begin_out[i] the largest start a with Lev = d for that end.  A C G T match the same letter in either case, every other byte matches nothing.
 * dist_out[i] = -1 (and begin = end = -1) where d > max_dist[i] or the read is longer than 65 536 bases.  Every job is checked before anything is
 * launched; MM_ERR_ARG with the broken rule as the message and the outputs untouched: a read or contig outside its set, a strand that is neither
 * +1 nor -1, a negative max_dist, a window that ends before it starts or lies outside its contig.  n_jobs == 0 is valid. */
int mm_edit_infix(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, int64_t n_jobs, const int32_t* read, const int32_t* strand,
                  const int32_t* contig, const int64_t* ws, const int64_t* we, const int32_t* max_dist,
                  int32_t* dist_out, int64_t* begin_out, int64_t* end_out);
/* The same for every record of a mapping, in mm_mapping_fetch order, the jobs made on the device: the window is contig[ws, we) with
 * pad = 64 + L / 16, ws = max(0, ref_start - pad), we = min(C, ref_start + L + pad), and max_dist = floor(1.5 L (100 - perc_identity) / 100).
 * dist_out[i] = d, first_out[i] = ws + a, last_out[i] = ws + b - 1 (0-based inclusive contig coordinates), or -1 -1 -1 where the record is not
 * aligned.  `reads` is the set that was mapped, `reference` the set whose contig numbering the records use; cap: room in the output arrays. */
int mm_mapping_edit_distances(mm_ctx* ctx, const mm_mapping* mapping, const mm_seqset* reads, const mm_seqset* reference, float perc_identity,
                              int32_t* dist_out, int64_t* first_out, int64_t* last_out, int64_t cap);

/* Base-level alignments of the same jobs ("Alignments"; the definition: csrc/mm_edit_core.hpp).  A job that is aligned has d, a,
 * b as above.  Let Q be the oriented read of length m, T = window[a, b) of length n, and E[i][j] the unit-cost edit distance of Q[i, m) to T[j, n)
 * (E[m][j] = n - j, E[i][n] = m - i, E[0][0] = d).  The alignment is the walk from (0, 0) to (m, n) that takes at each cell the first of
 *   =  if i < m, j < n and Q[i] matches T[j]           -> (i + 1, j + 1)
 *   X  if i < m, j < n and E[i+1][j+1] + 1 == E[i][j]  -> (i + 1, j + 1)
 *   I  if i < m and E[i+1][j] + 1 == E[i][j]           -> (i + 1, j)      (consumes a read base)
 *   D  otherwise                                       -> (i, j + 1)      (consumes a window base)
 * with equal neighbours merged into runs, each one 32-bit word as in BAM: len << 4 | op, I = 1, D = 2, = = 7, X = 8.  X + I + D bases = d,
 * = + X + I = m, = + X + D = n, at most 2 d + 1 runs, the first and the last never D.  A job that is not aligned, and an empty read, has no runs.
 * For strand -1 the runs are those of the reverse-complemented read along the forward contig (PAF's convention).
 * mm_edit_infix_align: the checks and messages of mm_edit_infix, nothing launched on a bad job.  mm_mapping_align: the
 * window and cap rules of mm_mapping_edit_distances.  dist / first / last are exactly what those two calls return for the same jobs (window
 * coordinates half-open for the former, 0-based inclusive contig coordinates for the latter, -1 -1 -1: not aligned).  The runs of job i are
 * ops[op_off[i], op_off[i + 1]).  The result lives in host memory until mm_alignment_destroy; no result depends on MM_EDIT_TRACE_MB. */
int mm_edit_infix_align(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, int64_t n_jobs, const int32_t* read, const int32_t* strand,
                        const int32_t* contig, const int64_t* ws, const int64_t* we, const int32_t* max_dist, mm_alignment** out);
int mm_mapping_align(mm_ctx* ctx, const mm_mapping* mapping, const mm_seqset* reads, const mm_seqset* reference, float perc_identity, mm_alignment** out);
int mm_alignment_sizes(const mm_alignment* al, int64_t* n_jobs, int64_t* n_ops);
int mm_alignment_fetch(const mm_alignment* al, int32_t* dist /* [n_jobs] */, int64_t* first, int64_t* last, int64_t* op_off /* [n_jobs + 1] */, uint32_t* ops /* [n_ops] */);
void mm_alignment_destroy(mm_alignment* al);

/* BAM records (SAM/BAM specification v1.6) of jobs that were aligned, encoded and deflated on the context's device ("BAM
 * output"; the record: csrc/mm_bam_core.hpp).  The arrays are the caller's: read / strand / contig name the jobs, dist / first / op_off / ops are
 * what mm_alignment_fetch gave for them (first: the 0-based contig coordinate of the alignment's first base), flag / mapq / names go into the
 * records as they are.  A job with dist < 0, and one whose read is empty, has no record.  A record: refID = contig, pos = first, bin =
 * reg2bin(first, first + reference span), l_seq = the read's length, next_refID = next_pos = -1, tlen = 0; the CIGAR is the runs as they are; SEQ
 * is the read as its set holds it (for strand -1 reversed, each 4-bit code of =ACMGRSVTWYHKDBN bit-reversed; a byte outside the table is N), QUAL is
 * the read's Phred bytes where its set carries qualities (mm_seqset_add_qual; reversed for strand -1), 0xFF on every base of a read without; the tags are NM:i (int32) = dist, MD:Z from the runs and the forward reference, and, for more than 65 535 runs, CG:B,I with the runs
 * while the CIGAR field holds <l_seq>S<span>N.  The records of consecutive jobs go into groups of at most group_bytes raw bytes (0: 255 MiB; a larger
 * record is a group of its own); each group is deflated where it was written and only its BGZF members come to the host, back to back.  The
 * inflated stream does not depend on group_bytes.  The file's header and the 28-byte end-of-file block are the caller's to write.
 * MM_ERR_ARG with "job <index>: rule <number>: ..." in mm_last_error, *out NULL and nothing written, for the lowest job that breaks a rule:
 *   1 a read or contig outside its set                      5 the = X I runs do not add up to the read's length
 *   2 a strand that is not +1 / -1, or flag & 0x10 that     6 first < 0, or first plus the = X D runs passes the contig's end
 *     disagrees with it                                     7 the X I D runs do not add up to dist
 *   3 a name of 0 or more than 254 bytes                    (rule 1 is asked of every job, the others of the jobs that have a record)
 *   4 a run whose op is not 1, 2, 7 or 8, or of length 0 */
int mm_bam_encode(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, int64_t n_jobs,
                  const int32_t* read, const int32_t* strand, const int32_t* contig,        /* the jobs that were aligned   */
                  const int32_t* dist, const int64_t* first,                                /* dist < 0: no record          */
                  const int64_t* op_off /* [n_jobs + 1] */, const uint32_t* ops,            /* as mm_alignment_fetch gives  */
                  const uint16_t* flag, const uint8_t* mapq,
                  const int64_t* name_off /* [n_jobs + 1] */, const char* names,
                  int64_t group_bytes, mm_bam** out);
int mm_bam_sizes(const mm_bam* bam, int64_t* n_records, int64_t* raw_bytes, int64_t* bgzf_bytes);
int mm_bam_fetch(const mm_bam* bam, uint8_t* bgzf /* [bgzf_bytes] */);
/* mm_bam_encode with the records of the call in ascending (contig, first, job index): a sorted run of a coordinate sort (DESIGN.md section 1,
 * "Sorted runs").  The same arguments, rules and refusals (the messages start with "mm_bam_encode_sorted"); every record is byte for byte the one
 * mm_bam_encode writes for its job.  The order is a stable radix sort of (contig << 32 | first, job) on the device; groups are cut along that order. */
int mm_bam_encode_sorted(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, int64_t n_jobs,
                         const int32_t* read, const int32_t* strand, const int32_t* contig,
                         const int32_t* dist, const int64_t* first,
                         const int64_t* op_off /* [n_jobs + 1] */, const uint32_t* ops,
                         const uint16_t* flag, const uint8_t* mapq,
                         const int64_t* name_off /* [n_jobs + 1] */, const char* names,
                         int64_t group_bytes, mm_bam** out);
/* The records of either encoder in the order of the inflated stream: record i belongs to job job[i] and lies at [raw_off[i], raw_off[i + 1]) of the
 * inflated bytes; raw_off[0] = 0 and raw_off[n_records] = raw_bytes. */
int mm_bam_fetch_records(const mm_bam* bam, int64_t* job /* [n_records] */, int64_t* raw_off /* [n_records + 1] */);
void mm_bam_destroy(mm_bam* bam);

/* FASTQ / FASTA records of selected reads of an uploaded set, written and deflated on the context's device (mapDirectly --extract-*; DESIGN.md
 * section 1, "Read extraction"; the record: csrc/mm_reads_out_core.hpp).  Record i is read read[i] of the set under the name names[name_off[i],
 * name_off[i + 1]); the indices come in any order and may repeat.  with_qual 1: "@name\nBASES\n+\nQUAL\n", QUAL the stored Phred values + 33 and '!'
 * on every base without a quality (a read added without qualities; a set without a quality plane, which is valid); with_qual 0: ">name\nBASES\n",
 * unwrapped.  BASES are the bytes the set holds, in the read's own orientation: upper-cased, bytes other than A C G T verbatim, nt16 codes as their
 * letters; an empty read gives empty lines.  The records of consecutive indices go into groups of at most group_bytes raw bytes (0: 255 MiB; a larger
 * record is a group of its own); each group is deflated where it was written and only its BGZF members come to the host, back to back.  The inflated
 * stream does not depend on group_bytes.  The 28-byte end-of-file block is the caller's to write.
 * MM_ERR_ARG with "mm_reads_encode: record <index>: rule <number>: ..." in mm_last_error, *out NULL and nothing written, for the lowest record that
 * breaks a rule (and its lowest rule):  1 a read outside the set;  2 a name of 0 or more than 254 bytes;  3 a name byte outside 0x21..0x7E.
 * MM_ERR_STATE for a set that is not uploaded and for a result of mm_seqset_hpc, which does not hold the reads' own bases. */
int mm_reads_encode(mm_ctx* ctx, const mm_seqset* reads, int64_t n_sel,
                    const int32_t* read,                                      /* indices into the set, any order, repeats allowed */
                    const int64_t* name_off /* [n_sel + 1] */, const char* names,
                    int with_qual,                                            /* 0: FASTA records, 1: FASTQ records */
                    int64_t group_bytes,                                      /* 0: 255 MiB */
                    mm_reads_text** out);
int mm_reads_text_sizes(const mm_reads_text* text, int64_t* n_records, int64_t* raw_bytes, int64_t* bgzf_bytes);
int mm_reads_text_fetch(const mm_reads_text* text, uint8_t* bgzf /* [bgzf_bytes] */);
void mm_reads_text_destroy(mm_reads_text* text);

/* The coordinate sort of BAM records: sorted runs (mm_bam_encode_sorted's members, one run per call) merged on the context's device into one stream of
 * BGZF members, and its BAI index ("Sorted BAM"; the definitions: csrc/mm_bam_sort_core.hpp).  The sorter never looks inside a
 * record: a record is raw_off[i + 1] - raw_off[i] bytes with the key (ref_id, pos) and the interval [pos, end), end = pos + max(1, reference span).
 *   create   ref_len: the contigs' lengths, each below 2^29 (BAI holds no coordinate beyond: MM_ERR_ARG).  window_bytes: the bytes of output made at
 *            a time, a multiple of 65280 up to 255 MiB; 0 is 255 MiB.  Device memory: two windows and two members per run, 40 bytes per record.
 *   add_run  the run's members back to back; they stay the caller's and must live until destroy.  raw_off: the records' offsets in the run's inflated
 *            bytes.  MM_ERR_ARG naming the run and the record: raw_off that does not start at 0, does not rise or does not end at the members' ISIZE sum;
 *            ref_id outside [0, n_ref); pos < 0; end not behind pos or past the contig's end; a run that is not ascending by (ref_id, pos).
 *            MM_ERR_DATA: a BSIZE chain that breaks.
 *   plan     after the last run: the number of windows and the stream's bytes.  The order is ascending (ref_id, pos), then run, then index in the run.
 *   window   w = 0, 1, ... in order (MM_ERR_STATE otherwise): the members of output bytes [w W, (w + 1) W), each of 65280 inflated bytes but the
 *            stream's last, fetched with mm_bam_sorter_fetch.  The members of all windows back to back do not depend on window_bytes.
 *            MM_ERR_DATA naming the run and the member: a member that does not inflate.
 *   index    after the last window: the bytes of the .bai for a file that holds header_bytes bytes of header members, the windows' members and the
 *            end-of-file block (the byte after the stream's last lies in that block at offset 0); fetched with mm_bam_sorter_fetch.  Per
 *            reference: the bins ascending, a bin's chunks the maximal runs of records that are neighbours in the file and share the bin, [vs of the
 *            first, ve of the last]; pseudo-bin 37450 with (vs of the reference's first record, ve of its last) and (its records, 0); the linear
 *            index of 1 + ((largest end - 1) >> 14) windows, window w holding the vs of the first record with pos < (w + 1) 2^14 and end > w 2^14,
 *            or else the next window's value; a reference without records has n_bin = n_intv = 0.  n_no_coor = 0 ends the file. */
int mm_bam_sorter_create(mm_ctx* ctx, int32_t n_ref, const int32_t* ref_len, int64_t window_bytes, mm_bam_sorter** out);
int mm_bam_sorter_add_run(mm_bam_sorter* s, const uint8_t* bgzf, int64_t bgzf_bytes, int64_t n_records, const int64_t* raw_off /* [n_records + 1] */,
                          const int32_t* ref_id, const int32_t* pos, const int32_t* end);
int mm_bam_sorter_plan(mm_bam_sorter* s, int64_t* n_windows, int64_t* stream_bytes);
int mm_bam_sorter_window(mm_bam_sorter* s, int64_t w, int64_t* bgzf_bytes);
int mm_bam_sorter_index(mm_bam_sorter* s, int64_t header_bytes, int64_t* bai_bytes);
int mm_bam_sorter_fetch(const mm_bam_sorter* s, uint8_t* out /* the bytes of the last window or index */);
void mm_bam_sorter_destroy(mm_bam_sorter* s);

/* The pileup of aligned jobs: what differs from the reference, counted per column on the context's device ("Pileup"; the
 * definition: csrc/mm_pileup_core.hpp).  A job contributes where use[i] != 0 and dist[i] >= 0.  Walking its runs from r = first, i = 0 in the oriented
 * read Q: an = run gives nothing; an X run of n the events (contig, r + t, code(Q[i + t])), A 0 C 1 G 2 T 3, any other byte N 4; a D run of n the events
 * (contig, r + t, 5); an I run ONE event (contig, r > first ? r - 1 : first, 6): the base before the insertion, `first` for a leading one.
 * key = contig << 35 | pos << 3 | code (2^29 contigs at most: MM_ERR_ARG beyond), so keys order by contig, position, code.
 * mm_pileup_events returns the events of one call's jobs as (key, count) pairs with unique keys in ascending order.  It applies mm_bam_encode's rules
 * 1, 2 (the strand), 4, 5 and 6 to the jobs it uses: MM_ERR_ARG with "mm_pileup_events: job <index>: rule <number>: ..." for the lowest offender.
 * mm_pileup_merge takes any multiset of pairs (unsorted, keys may repeat) and returns the table with equal keys summed; a sum above 2^32 - 1 is
 * MM_ERR_ARG.  mm_pileup_finish takes a merged table (keys ascending and unique, every key a position of `reference`: MM_ERR_ARG otherwise) and the
 * intervals [iv_first, iv_last] on iv_contig of EVERY contributing alignment of the run: depth(contig, pos) is the number of intervals that hold pos;
 * an entry is kept where count >= min_count && (double)count >= min_frac * (double)depth, and carries the reference's byte at its position.  Per contig:
 * alignments (its intervals), covered (positions of depth >= 1: the length of the intervals' union) and sum_depth (the sum of last - first + 1).
 * All arrays are the caller's; results live in host memory until destroyed; an error leaves *out NULL and launches nothing further. */
int mm_pileup_events(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, int64_t n_jobs,
                     const int32_t* read, const int32_t* strand, const int32_t* contig, const int32_t* dist, const int64_t* first,
                     const int64_t* op_off /* [n_jobs + 1] */, const uint32_t* ops, const uint8_t* use /* [n_jobs] */, mm_pileup** out);
/* The same under a base-quality floor min_base_quality (0..93: MM_ERR_ARG otherwise; 0 is mm_pileup_events bit for bit, and so is any floor on reads
 * without qualities: "no quality" counts as 255).  With q(i) the quality of base i of the oriented read of m bases: the event of an X run at read
 * index i + t is kept iff q(i + t) >= floor; the events of a D run met at read index i are kept together iff min(q(i - 1) if i > 0, q(i) if i < m) >=
 * floor; the event of an I run of n iff min q(i .. i + n - 1) >= floor.  The table holds exactly the kept events.  Intervals, and so depth, do not
 * depend on the floor. */
int mm_pileup_events_q(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, int64_t n_jobs,
                       const int32_t* read, const int32_t* strand, const int32_t* contig, const int32_t* dist, const int64_t* first,
                       const int64_t* op_off /* [n_jobs + 1] */, const uint32_t* ops, const uint8_t* use /* [n_jobs] */, int32_t min_base_quality,
                       mm_pileup** out);
int mm_pileup_merge(mm_ctx* ctx, int64_t n, const uint64_t* keys, const uint32_t* counts, mm_pileup** out);
int mm_pileup_sizes(const mm_pileup* table, int64_t* n_pairs);
int mm_pileup_fetch(const mm_pileup* table, uint64_t* keys /* [n_pairs] */, uint32_t* counts);
void mm_pileup_destroy(mm_pileup* table);
int mm_pileup_finish(mm_ctx* ctx, const mm_seqset* reference, int64_t n, const uint64_t* keys, const uint32_t* counts,
                     int64_t n_iv, const int32_t* iv_contig, const int64_t* iv_first, const int64_t* iv_last,
                     int64_t min_count, double min_frac, mm_pileup_result** out);
int mm_pileup_result_sizes(const mm_pileup_result* result, int64_t* n_sites, int64_t* n_contigs);
int mm_pileup_result_fetch_sites(const mm_pileup_result* result, uint64_t* key /* [n_sites] */, uint32_t* count, uint32_t* depth, uint8_t* ref_byte);
int mm_pileup_result_fetch_contigs(const mm_pileup_result* result, int64_t* alignments /* [n_contigs] */, int64_t* covered, int64_t* sum_depth);
void mm_pileup_result_destroy(mm_pileup_result* result);

/* The modification calls of aligned jobs per reference position and strand ("Base modifications"; the definition:
 * csrc/mm_mods_core.hpp).  A job contributes where use[i] != 0 and dist[i] >= 0, as in mm_pileup_events.  Walking its runs from r = first, i = 0:
 * column t of an = run reads the stored base s = i + t (strand +1) or m - 1 - (i + t) (strand -1) of its read of m bases; where who[s] != 0 it gives
 * one event (contig, r + t, strand, class) with class 1 (fail) if prob[s] < min_ml, else 0 for canonical, 2 for another code, 3 + code.  X, I and D
 * runs give none; a read without groups and a set without a plane give none.  key = contig << 36 | pos << 4 | (strand < 0) << 3 | class; more than
 * 2^28 contigs is MM_ERR_ARG, and so is min_ml outside [0, 255].  mm_mod_events returns one call's events as (key, count) pairs with unique keys in
 * ascending order and applies mm_bam_encode's rules 1, 2 (the strand), 4, 5 and 6 to the jobs it uses: MM_ERR_ARG with "mm_mod_events: job <index>:
 * rule <number>: ..." for the lowest offender.  mm_mod_merge takes any multiset of pairs and returns the table with equal keys summed; a sum above
 * 2^32 - 1 is MM_ERR_ARG.  mm_mod_finish takes a merged table (keys ascending and unique, every key a position of `reference` and a class below
 * 3 + n_codes: MM_ERR_ARG otherwise), the base letter of each of the 1..4 asked codes and min_coverage >= 1.  At (contig, pos, strand), with b the
 * reference's byte, upper-cased, complemented for strand -1 (a b outside ACGT gives no row), every code k whose base is b gives, in the codes' order,
 * a row with N_mod = the count of class 3 + k, N_canonical = class 0, N_other = class 2 plus the other asked codes, N_fail = class 1; it is kept iff
 * N_mod + N_canonical + N_other >= min_coverage.  Rows come in the order contig, pos, + before -, code; site = key with k in the place of the class.
 * The tables and results are host memory. */
typedef struct mm_mod mm_mod;                 /* a table of (key, count) modification events, unique keys ascending */
typedef struct mm_mod_result mm_mod_result;   /* the rows of a run's modification table */
int mm_mod_events(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, int64_t n_jobs,
                  const int32_t* read, const int32_t* strand, const int32_t* contig, const int32_t* dist, const int64_t* first,
                  const int64_t* op_off /* [n_jobs + 1] */, const uint32_t* ops, const uint8_t* use /* [n_jobs] */, int32_t min_ml, mm_mod** out);
int mm_mod_merge(mm_ctx* ctx, int64_t n, const uint64_t* keys, const uint32_t* counts, mm_mod** out);
int mm_mod_sizes(const mm_mod* table, int64_t* n_pairs);
int mm_mod_fetch(const mm_mod* table, uint64_t* keys /* [n_pairs] */, uint32_t* counts);
void mm_mod_destroy(mm_mod* table);
int mm_mod_finish(mm_ctx* ctx, const mm_seqset* reference, int64_t n, const uint64_t* keys, const uint32_t* counts,
                  int32_t n_codes, const uint8_t* code_base /* [n_codes] */, int64_t min_coverage, mm_mod_result** out);
int mm_mod_result_sizes(const mm_mod_result* result, int64_t* n_rows);
int mm_mod_result_fetch(const mm_mod_result* result, uint64_t* site /* [n_rows] */, uint64_t* n_mod, uint64_t* n_canonical, uint64_t* n_other, uint64_t* n_fail);
void mm_mod_result_destroy(mm_mod_result* result);

/* Methylation per sequence motif over the contigs [contig_lo, contig_hi) ("Modification motifs"; the definition:
 * csrc/mm_motif_core.hpp).  The table, the codes and min_coverage are mm_mod_finish's, with the same checks; only the keys of the group's contigs
 * contribute.  Motif j has the letters motif_mask[motif_off[j], motif_off[j + 1]) as 4-bit sets (A 1, C 2, G 4, T 8, IUPAC letters their unions) and its
 * modified base at motif_pos[j]: a length outside 1..32, a mask outside 1..15, a modified base that is not a one-bit mask inside the motif, n_motifs outside
 * 1..8 and, under combine_strands, a motif that is not its own reverse complement are MM_ERR_ARG with "mm_mod_motifs: motif <index>: ...".  A reference byte
 * outside A C G T fits no letter; no occurrence crosses a contig's end.  An occurrence with modified position q on a strand takes, for every code whose base
 * is the motif's modified base, mm_mod_finish's counts at (contig, q, strand), zero without an entry; it is covered iff N_mod + N_canonical + N_other >=
 * min_coverage and modified iff covered and N_mod >= min_frac (0..1) of that sum.  Under combine_strands the + and - occurrence of one window are one unit at
 * the + site with the sums of both.  Rows: the covered (occurrence, code) in the order contig, position, + before -, motif, code; site = contig << 36 |
 * pos << 4 | (strand < 0) << 3 (a unit: strand bit 0).  Summary: one entry per (contig with an entry in the table, motif, applicable code) in that order
 * with MM_MOTIF_SUMS sums: sites (all occurrences, or units), covered, modified, N_valid_cov and N_mod over the covered ones.  The rows and summaries of
 * successive groups, one behind the other, are those of one call over all contigs.  The result is host memory. */
#define MM_MOTIF_SUMS 5
typedef struct mm_motif_result mm_motif_result;
int mm_mod_motifs(mm_ctx* ctx, const mm_seqset* reference, int32_t contig_lo, int32_t contig_hi, int64_t n, const uint64_t* keys, const uint32_t* counts,
                  int32_t n_codes, const uint8_t* code_base /* [n_codes] */, int32_t n_motifs, const int32_t* motif_off /* [n_motifs + 1] */,
                  const uint8_t* motif_mask, const int32_t* motif_pos /* [n_motifs] */, int64_t min_coverage, double min_frac, int32_t combine_strands,
                  mm_motif_result** out);
int mm_motif_result_sizes(const mm_motif_result* result, int64_t* n_rows, int64_t* n_summary);
int mm_motif_result_fetch_rows(const mm_motif_result* result, uint64_t* site /* [n_rows] */, int32_t* motif, int32_t* code, uint64_t* n_mod, uint64_t* n_canonical,
                               uint64_t* n_other, uint64_t* n_fail);
int mm_motif_result_fetch_summary(const mm_motif_result* result, int32_t* contig /* [n_summary] */, int32_t* motif, int32_t* code, int64_t* sums /* [MM_MOTIF_SUMS * n_summary] */);
void mm_motif_result_destroy(mm_motif_result* result);

/* The alleles of aligned jobs: SNVs, deletions and insertions that are canonical across reads, left-aligned and counted on the context's device (DESIGN.md
 * section 1, "VCF"; the definition: csrc/mm_vcf_core.hpp).  A job contributes where use[i] != 0 and dist[i] >= 0.  Walking its runs from r = first, i = 0
 * in the oriented read Q, with last its last contig position: an X run of n gives an SNV (contig, r + t, code(Q[i + t])) per base of A C G T; a D run of n
 * with first < r and r + n <= last a deletion of n anchored at a = r - 1; an I run of n with first < r <= last whose bases are all A C G T an insertion of
 * S = Q[i .. i + n) anchored at a = r - 1.  Indel runs at an end of the alignment are edges, not alleles.  An indel is shifted left, at most 256 times:
 * a deletion while a > first and ref[a] == ref[a + n], an insertion while a > first and ref[a] == the last base of S, which then turns right by one; a
 * reference byte outside A C G T stops the shift.  Key: w0 = contig << 35 | pos << 3 | code (code: the alt's 0-3, 5 deletion, 6 insertion; pos: the SNV's
 * position or the shifted anchor), w1 = 0 (SNV), n (deletion), n << 48 | the bases 2 bits each, base j at bits 2j (insertion, n <= 24), n << 48
 * (insertion, n > 24: symbolic).  Keys order by (w0, w1).
 * mm_vcf_events returns the alleles of one call's jobs as (w0, w1, count) triples with unique keys in ascending order.  It applies mm_bam_encode's rules
 * 1, 2, 4, 5 and 6 and rule 8 (an I or D run between other runs of 2^16 bases or more) to the jobs it uses: MM_ERR_ARG with "mm_vcf_events: job <index>:
 * rule <number>: ..." for the lowest offender.  mm_vcf_merge takes any multiset of triples and returns the table with equal keys summed; a sum above
 * 2^32 - 1 is MM_ERR_ARG.  mm_vcf_finish takes a merged table (keys ascending and unique, every key an allele on `reference`: MM_ERR_ARG otherwise) and the
 * intervals of EVERY contributing alignment of the run, as mm_pileup_finish does: depth is the number of intervals that hold pos; an allele is kept where
 * count >= min_count && (double)count >= min_frac * (double)depth, and carries MM_VCF_WINDOW reference bytes from pos on (0 beyond the contig's end).
 * All arrays are the caller's; results live in host memory until destroyed; an error leaves *out NULL and launches nothing further. */
#define MM_VCF_WINDOW 25
int mm_vcf_events(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, int64_t n_jobs,
                  const int32_t* read, const int32_t* strand, const int32_t* contig, const int32_t* dist, const int64_t* first,
                  const int64_t* op_off /* [n_jobs + 1] */, const uint32_t* ops, const uint8_t* use /* [n_jobs] */, mm_vcf** out);
/* The same under mm_pileup_events_q's base-quality floor: an SNV, a deletion and an insertion are kept by the rules of the X, D and I run they come
 * from, asked before the left shift, which acts on the alleles that were kept.  The rules' checks are unchanged. */
int mm_vcf_events_q(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, int64_t n_jobs,
                    const int32_t* read, const int32_t* strand, const int32_t* contig, const int32_t* dist, const int64_t* first,
                    const int64_t* op_off /* [n_jobs + 1] */, const uint32_t* ops, const uint8_t* use /* [n_jobs] */, int32_t min_base_quality,
                    mm_vcf** out);
int mm_vcf_merge(mm_ctx* ctx, int64_t n, const uint64_t* w0, const uint64_t* w1, const uint32_t* counts, mm_vcf** out);
int mm_vcf_sizes(const mm_vcf* table, int64_t* n_triples);
int mm_vcf_fetch(const mm_vcf* table, uint64_t* w0 /* [n_triples] */, uint64_t* w1, uint32_t* counts);
void mm_vcf_destroy(mm_vcf* table);
int mm_vcf_finish(mm_ctx* ctx, const mm_seqset* reference, int64_t n, const uint64_t* w0, const uint64_t* w1, const uint32_t* counts,
                  int64_t n_iv, const int32_t* iv_contig, const int64_t* iv_first, const int64_t* iv_last,
                  int64_t min_count, double min_frac, mm_vcf_result** out);
int mm_vcf_result_sizes(const mm_vcf_result* result, int64_t* n_alleles);
int mm_vcf_result_fetch(const mm_vcf_result* result, uint64_t* w0 /* [n_alleles] */, uint64_t* w1, uint32_t* count, uint32_t* depth,
                        uint8_t* window /* [MM_VCF_WINDOW * n_alleles] */);
void mm_vcf_result_destroy(mm_vcf_result* result);

/* The consensus of the contigs [contig_lo, contig_hi) of `reference`: the sequence of the strain the reads come from, built on the context's device from a
 * merged mm_vcf table and the intervals of EVERY contributing alignment ("Consensus"; the definition: csrc/mm_cons_core.hpp).  One call
 * handles one group of contigs, and its device and host memory are bounded by the group's bases.  depth(c, p) is the number of intervals that hold p; p is
 * called where depth >= min_depth.  A row is a candidate where depth(c, pos) >= min_depth && (double)count >= min_frac * (double)depth.  Candidates are taken
 * per contig in key order: a deletion (anchor a, length n, footprint [a + 1, a + n]) is applied iff a + 1 lies behind the footprint end of every earlier
 * candidate deletion, applied or not (of [10, 20], [15, 25] and [22, 30] only the first is applied; abutting deletions both are); an SNV or an insertion is
 * applied iff its position is in no applied footprint and no earlier candidate of its kind sits there.  Per position the consensus holds nothing (deleted),
 * or the applied SNV's alt, else N where the position is not called, else the reference's base (N for a byte outside A C G T); then the bases of an insertion
 * applied there (n times N for an insertion of more than 24 bases, whose bases the key does not hold).  Per contig with an interval there are MM_CONS_STATS
 * counters: alignments, called, written, consensusLength, snvs, deletions, deletedBases, insertions, insertedBases, dropped (candidates that were not
 * applied).  A contig is written iff called >= max(1, ceil(min_called * length)); its consensusLength is 0 otherwise.  The text of a written contig is its
 * bytes in lines of line_width, every line followed by \n.
 * MM_ERR_ARG: min_depth < 1, min_frac outside [0.5, 1], min_called outside [0, 1], line_width < 1, a table that is not merged or holds a key that is no allele
 * on `reference`, a row or an interval on a contig outside the range.  All of this is checked on the host before anything is launched.  All arrays are the
 * caller's; the result lives in host memory until destroyed; an error leaves *out NULL and launches nothing further.  MM_CONS_TIMING=1 prints the stages'
 * device times. */
#define MM_CONS_STATS 10
int mm_consensus(mm_ctx* ctx, const mm_seqset* reference, int32_t contig_lo, int32_t contig_hi,
                 int64_t n, const uint64_t* w0, const uint64_t* w1, const uint32_t* counts,
                 int64_t n_iv, const int32_t* iv_contig, const int64_t* iv_first, const int64_t* iv_last,
                 int64_t min_depth, double min_frac, double min_called, int32_t line_width, struct mm_consensus** out);
/* n_contigs: the group's contigs with an interval; n_written: those of them that are written; text_bytes: the bytes of their texts together */
int mm_consensus_sizes(const struct mm_consensus* result, int64_t* n_contigs, int64_t* n_written, int64_t* text_bytes);
/* the contigs with an interval, ascending, and their counters in the order given above */
int mm_consensus_fetch_contigs(const struct mm_consensus* result, int32_t* contig /* [n_contigs] */, int64_t* stats /* [MM_CONS_STATS * n_contigs] */);
/* the written contigs, ascending; the text of contig[j] is text[text_off[j], text_off[j + 1]) */
int mm_consensus_fetch_text(const struct mm_consensus* result, int32_t* contig /* [n_written] */, int64_t* text_off /* [n_written + 1] */, uint8_t* text /* [text_bytes] */);
void mm_consensus_destroy(struct mm_consensus* result);

/* The depth profile of n_iv intervals (contig, first, last) over contigs of the given LENGTHS, computed on the context's device ("Depth";
 * the definition: csrc/mm_depth_core.hpp).  The call reads no base and keeps no array indexed by a reference position: depth changes only at the 2 n_iv interval
 * ends, so device and host memory are O(n_iv + listed contigs + windows) whatever the contigs' lengths.  depth(c, p) is the number of intervals that hold p
 * (mm_pileup_finish's depth); nothing depends on the order of the intervals.
 *   runs     the maximal [start, end) of equal depth >= 1 inside one contig, ordered by contig, then start; neighbouring pieces of equal depth are one run
 *            ([0,4] and [5,9] at depth 1 give [0,10)), a run never crosses a contig's end, and zero depth is not listed.
 *   contigs  for every contig with an interval, ascending, MM_DEPTH_STATS counters: alignments, covered, sumDepth (the three of mm_pileup_finish), medianDepth
 *            (the depth at rank (len - 1) / 2, 0-based, of the contig's len depths sorted ascending, zeros included), maxDepth; then n_thresholds counters ge[t],
 *            the positions with depth >= thresholds[t].
 *   windows  for every such contig all windows [k * window, min((k + 1) * window, len)), k < ceil(len / window), each with the sum of its depths and its covered
 *            positions; win_off[j] is the first window of the j-th listed contig, win_off[n_contigs] their number.
 * All sums are 64-bit, a depth is 32-bit.  MM_ERR_ARG: a length outside [1, 2^29), more than 2^29 contigs, an interval off its contig or with first > last (the
 * message names the lowest one), window < 1, more than 8 thresholds, a threshold < 1, thresholds that are not strictly ascending, more than 2^31 - 1 windows
 * (the message names the window).  MM_ERR_LIMIT: 2^31 intervals or more.  All of this is checked on the host before anything is launched; n_iv == 0 gives an
 * empty result and launches nothing.  All arrays are the caller's; the result lives in host memory until destroyed; an error leaves *out NULL.
 * MM_DEPTH_TIMING=1 prints the stages' device times. */
#define MM_DEPTH_STATS 5   /* alignments, covered, sumDepth, medianDepth, maxDepth; then n_thresholds ge counters */
typedef struct mm_depth mm_depth;
int mm_depth_profile(mm_ctx* ctx, int64_t n_contigs, const int64_t* contig_len,
                     int64_t n_iv, const int32_t* iv_contig, const int64_t* iv_first, const int64_t* iv_last,
                     int64_t window, int32_t n_thresholds, const int64_t* thresholds, mm_depth** out);
/* n_contigs: the contigs with an interval */
int mm_depth_sizes(const mm_depth* result, int64_t* n_runs, int64_t* n_contigs, int64_t* n_windows);
int mm_depth_fetch_runs(const mm_depth* result, int32_t* contig /* [n_runs] */, int64_t* start, int64_t* end, uint32_t* depth);
int mm_depth_fetch_contigs(const mm_depth* result, int32_t* contig /* [n_contigs] */, int64_t* win_off /* [n_contigs + 1] */,
                           int64_t* stats /* [(MM_DEPTH_STATS + n_thresholds) * n_contigs] */);
int mm_depth_fetch_windows(const mm_depth* result, int64_t* sum /* [n_windows] */, int64_t* covered /* [n_windows] */);
void mm_depth_destroy(mm_depth* result);

/* The error profile of aligned jobs ("Error profile"; the definition: csrc/mm_errprof_core.hpp): what the jobs with use != 0 and
 * dist >= 0 say about the reads, walked on the context's device.  The jobs are mm_pileup_events' (the runs of mm_alignment_fetch, len << 4 | op) and so are
 * the rules, mm_bam_encode's 1, 2 (the strand), 4, 5 and 6.  The walk runs from r = first, i = 0 over the oriented read Q (the reverse complement for strand -1)
 * with q(i) its quality (0xFF: none) and code A 0 C 1 G 2 T 3, else N 4:
 *   = or X column at (r, i)  counted in the read's orientation, as the sequencer saw it: truth a = code(R[r]) (its complement for strand -1), observed b = the
 *                            code of the stored read byte; SUB[a * 5 + b] += 1 and QUAL[cls][row(q(i))] += 1, cls 0 for =, 1 for X; row(q) = q for 0..93, 94 for none.
 *   I run of n at (r, i)     QUAL[2][row(q(i + t))] += 1 for each base; INDEL[0][hp][min(n, 64) - 1] += 1, hp = 1 iff the n oriented bases are one letter b of
 *                            A C G T and R[r - 1] == b (r >= 1) or R[r] == b (r < the contig's length).
 *   D run of n at r          INDEL[1][hp][min(n, 64) - 1] += 1, hp = 1 iff R[r .. r + n) is one letter b of A C G T and R[r - 1] == b (r >= 1) or R[r + n] == b
 *                            (r + n < the contig's length).
 * counters: MM_ERRPROF_COUNTERS 64-bit sums in the order SUB[25], INDEL[kind][hp][64], QUAL[cls][95], overwritten.  cols: per job eq, x, insRuns, insBases,
 * delRuns, delBases (zeros for a job that is not used).  ident_key: per job contig << 32 | ppm with ppm = floor(10^6 * eq / (eq + x + insBases + delBases)) in
 * 64-bit integers (0 for an empty read), ~0 for a job that is not used.  All results are integers that add across calls, so nothing depends on batches,
 * devices or order.  MM_ERR_ARG "mm_errprof_events: job <index>: rule <n>: ..." names the lowest job that breaks a rule; the outputs are then unspecified.
 * n_jobs == 0 gives zero counters and launches nothing.  All arrays are the caller's.  The walk runs in MM_ERRPROF_GROUPS workgroups (default: 16 per CU), each
 * with its counters in LDS and one row of partial sums; MM_ERRPROF_TIMING=1 prints the stages' device times. */
#define MM_ERRPROF_COUNTERS 566   /* 25 + 2 * 2 * 64 + 3 * 95 */
#define MM_ERRPROF_COLS 6         /* eq, x, insRuns, insBases, delRuns, delBases */
int mm_errprof_events(mm_ctx* ctx, const mm_seqset* reads, const mm_seqset* reference, int64_t n_jobs, const int32_t* read, const int32_t* strand,
                      const int32_t* contig, const int32_t* dist, const int64_t* first, const int64_t* op_off, const uint32_t* ops, const uint8_t* use,
                      uint64_t* counters /* [MM_ERRPROF_COUNTERS], overwritten */, int32_t* cols /* [n_jobs][MM_ERRPROF_COLS] */, uint64_t* ident_key /* [n_jobs] */);
/* The per-contig rows of a query file's error profile from the (ident_key, cols) of all its contributing alignments, in any order; entries whose key is ~0 are
 * skipped.  On the device: one sort of (key, index), the segment of every contig by binary searches, and per contig with at least one alignment
 * MM_ERRPROF_STATS values: alignments, the six column sums, and of its ppm values v[0 .. n) sorted ascending min = v[0], q1 = v[(n - 1) / 4],
 * median = v[(n - 1) / 2], q3 = v[3 (n - 1) / 4] (integer divisions), max = v[n - 1].  One more row holds the same over all alignments together (zeros
 * without any).  MM_ERR_ARG: a key whose contig is >= n_contigs (the message names the lowest entry), a negative count, a null array; checked before anything is
 * launched; an error leaves *out NULL; n == 0 launches nothing.  The result lives in host memory until destroyed. */
#define MM_ERRPROF_STATS 12   /* alignments, eq, x, insRuns, insBases, delRuns, delBases, min, q1, median, q3, max (ppm) */
typedef struct mm_errprof mm_errprof;
int mm_errprof_finish(mm_ctx* ctx, int64_t n_contigs, int64_t n, const uint64_t* ident_key /* [n] */, const int32_t* cols /* [n][MM_ERRPROF_COLS] */, mm_errprof** out);
/* n_contigs: the contigs with an alignment */
int mm_errprof_sizes(const mm_errprof* result, int64_t* n_contigs);
int mm_errprof_fetch(const mm_errprof* result, int32_t* contig /* [n_contigs], ascending */, int64_t* stats /* [(n_contigs + 1) * MM_ERRPROF_STATS]: the last row is all alignments' */);
void mm_errprof_destroy(mm_errprof* result);

/* ---- communicator (RCCL over xGMI; one process per GPU) --------------------------------------- */
#define MM_COMM_ID_BYTES 128
int mm_comm_unique_id(char id[MM_COMM_ID_BYTES]);                     /* rank 0 creates, caller broadcasts */
int mm_comm_init(mm_ctx* ctx, const char id[MM_COMM_ID_BYTES], int rank, int nranks);
/* what RCCL itself says about ctx's communicator (ncclCommCount / ncclCommUserRank); 1 / 0 without one */
int mm_comm_info(mm_ctx* ctx, int* n_ranks, int* rank);
/* Several contexts of one device (e.g. two host threads that take read batches in turn) use ONE communicator: `ctx` borrows the
 * communicator of `owner` (same device; the owner outlives it).  The caller issues the collectives of the sharing contexts in
 * the same order on every rank. */
int mm_comm_share(mm_ctx* ctx, mm_ctx* owner);
int mm_comm_allreduce_f64(mm_ctx* ctx, double* host_inout, int64_t n);   /* staging helper for small vectors */
void mm_comm_destroy(mm_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* METAMAPS_HIP_H */
