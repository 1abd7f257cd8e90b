// `metamaps` — drop-in command line front end for the MI355X hot path.
//
// Keeps the reference's sub-commands, flags and on-disk formats (map/include/parseCmdArgs.hpp:33-117,
// map/mash_map.cpp:257-317; files: map/mapWrap.h:39-211, meta/fEM.h:663-803) and drives the device
// exclusively through the C ABI in include/metamaps_hip.h.  Host work here is what stays host work in the
// reference too: argument parsing, FASTA/FASTQ(.gz) reading, text formatting, taxonomy bookkeeping.
//
//   metamaps mapDirectly [--all] [--compress-output] [--edit-distance] [--paf] [--bam] [--bam-sorted] [--pileup [--pileup-min-count N] [--pileup-min-frac F]]
//                       [--vcf [--vcf-min-count N] [--vcf-min-frac F]]
//                       [--consensus [--consensus-min-depth D] [--consensus-min-frac F] [--consensus-min-called C]] [--mods LIST [--mod-min-ml T] [--mod-min-coverage N] [--mod-motifs M1,M2,...]]
//                       [--depth [--depth-window W] [--depth-thresholds T1,T2,...]] [--error-profile]
//                       [--extract-unmapped] [--extract-mapped] [--extract-taxa ID[,ID...]] [--deplete-taxa ID[,ID...]]
//                        -r DB.fa -q reads.{fq,fa,fq.gz,bam} -o PREFIX [-k 16] [-w W] [-m 1000] [--pi 80] [-p 1e-3] [-t N] [--mm G] [--gpus N]
//   metamaps index -r DB.fa -i IDX [same reference options]          metamaps mapAgainstIndex [--all] -i IDX -q reads.fq -o PREFIX [--gpus N]
//   metamaps classify --DB DBDIR --mappings PREFIX [--minreads N] [-t N] [--gpus N] [--bootstrap B [--bootstrap-seed S]] [--lca T] [--genes] [--min-identity T [--refit]]
//
// --gpus N uses devices 0..N-1 of the node, one context per device on its own host thread (where the reference has -t N worker
// threads, computeMap.hpp:104-176 / fEM.h:1229): mapping shards the read batches (index replicated) or the index chunks
// (--shard-index / --stream-chunks) over the devices and writes the output in input order; classify shards the reads and
// all-reduces the per-taxon EM sums over RCCL every iteration.  (--devices a,b,c names the devices explicitly; a device may
// repeat — several contexts on one GPU — which is how the multi-device paths are tested on a one-GPU box.)
//
// --mm G splits the reference into the same index chunks the reference would build under that limit
// (mm_index_plan_chunks); all chunk indexes stay resident in HBM and every read batch is mapped against each.
// (--maxmemory-bytes N gives the limit in bytes: a test hook, sub-GiB limits make small references chunk.)
// --stream-chunks (automatic when the chunk indexes cannot all be resident): one chunk index on the device at a time,
// every read batch (kept packed on the device) mapped against it, merge at the end — mapWrap.h:417-437 with HBM in
// place of the PREFIX.N files.  (--stream-range-bases N: test hook, size of the contig ranges the chunk rule is evaluated on.)
//
// `index` stores the packed reference per chunk (own versioned format, include/metamaps_hip.h: mm_seqset_save) instead of
// the reference's Boost archives of the sketch; the device index is rebuilt from it in seconds.  `index --full-index` stores the
// device index itself (IDX.N.mmidx, mm_index_save: the arrays as they lie in HBM) and mapAgainstIndex loads it without running a
// kernel — the persistent index of SURVEY N2; which of the two is faster is a question of file bandwidth against build time.
//
// Query files (-q) may be FASTA/FASTQ(.gz) or BAM, recognised by content, per file of a comma list (host/bam_reader.hpp).  A BAM gives the
// files its `samtools fastq -n` conversion gives: secondary and supplementary records skipped, 0x10 records turned back to the read as
// sequenced, qualities, tags and paired-end flags ignored.  Its 4-bit codes are packed on the device (mm_seqset_add_nt16).  The BGZF blocks
// of FASTA/FASTQ written by bgzip (and of a BAM with MM_BAM_DEVICE_INFLATE=1) are inflated on the device a segment at a time
// (mm_bgzf_inflate); the host walks the block headers, cuts the records and parses the text.  Plain gzip FASTA/FASTQ — queries and the reference
// (-r DB.fa.gz) — is inflated on the device too, by speculative decoding of chunks of the one DEFLATE stream (mm_gzip_*); the
// parse is the zlib reader's.  MM_GZIP_HOST_INFLATE=1 keeps zlib's sequential reader.  The reference (-r) stays FASTA/FASTQ(.gz).
//
// --compress-output (mapDirectly, mapAgainstIndex; not in the reference): the mappings go to PREFIX.gz as BGZF, ending in BGZF's end-of-file
// block, and no plain PREFIX is written (one left by an earlier run is removed); .meta, .meta.unmappedReadsLengths and .parameters are as ever.
// The text of a batch is deflated on the device by the context that mapped it (mm_bgzf_deflate; MM_DEFLATE_HOST=1: zlib level 1 on the host)
// and the writer concatenates the batches' members.  `classify --mappings PREFIX` takes PREFIX if it exists (inflated if it starts with a
// BGZF block) and PREFIX.gz otherwise: the block headers are walked on the host, the blocks inflated on the device (mm_bgzf_inflate) into
// the buffer the tokeniser works on; any bgzip'd mappings file is accepted.  A corrupt or truncated file ends the run with the compressed
// offset of the bad block.  A plain gzip mappings file (no BGZF blocks) is refused with a message that says so.
//
// --edit-distance (mapDirectly; not in the reference): PREFIX.editDistances beside PREFIX, one line per mapping line in the same order,
// "readID contigID strand d first last": the exact unit-cost edit distance of the whole read (its reverse complement for strand -) to the best
// substring of the window contig[ref_start - pad, ref_start + L + pad), pad = 64 + L / 16, and that substring's 0-based inclusive coordinates;
// "NA NA NA" where the distance is above floor(1.5 L (100 - pi) / 100) or the read is longer than 65 536 bases.  Aligned on the device that mapped
// the batch (mm_mapping_edit_distances, host/batch_outputs.hpp); every device keeps its packed reference (0.25 bytes per base) and a batch's reads live
// until its distances are fetched.  PREFIX, .meta* and .parameters are the bytes of a run without the flag.  Refused: --hpc, index, mapAgainstIndex,
// classify, and any run whose chunk indexes are sharded or streamed (--shard-index, --stream-chunks, or an index that does not fit one device).
//
// --paf (mapDirectly; not in the reference; implies --edit-distance): also PREFIX.paf, one PAF line per ALIGNED line of PREFIX in the same order,
// "readID L 0 L strand contigID contigLen first last+1 matches alignmentLength 255 NM:i:d cg:Z:CIGAR" with = X I D runs: the base-level alignment
// behind d, first and last (the definition: csrc/mm_edit_core.hpp; for strand - the reverse-complemented read along the forward contig).  The context
// that mapped a batch traces it on the device in the one call that also gives the .editDistances lines (mm_mapping_align, host/batch_outputs.hpp).  A mapping
// that is not aligned has no PAF line.  PREFIX.paf is plain text even under --compress-output.  Refused wherever --edit-distance is.
//
// --bam (mapDirectly; not in the reference; implies --edit-distance; may be combined with --paf): also PREFIX.bam, one BAM record (SAM/BAM specification
// v1.6) per ALIGNED line of PREFIX in the same order, unsorted, a read's records together (GO:query): the CIGAR of = X I D runs, NM, MD, the read's bases
// (for strand - reverse-complemented) and 0xFF qualities (the read's own under --base-qualities); mapq from the printed field 14 of the record's line, 0x100 on every record of a read but the one
// with the largest field 14 (host/bam_out.hpp).  The device that mapped a batch encodes its records from the alignment the .editDistances and .paf lines
// come from and deflates them where they lie (mm_bam_encode); the file is BGZF whatever --compress-output says and ends with the end-of-file block.
// Every other file of the run is the file of the same run without the flag.  Refused wherever --edit-distance is.
//
// --bam-sorted (mapDirectly; not in the reference; implies --edit-distance; with or without --bam and every other side output): also PREFIX.sorted.bam, the
// records of PREFIX.bam in ascending (refID, pos, place in PREFIX.bam) in BGZF members of 65 280 bytes, and PREFIX.sorted.bam.bai (bam_sort_out.hpp); refused
// wherever --edit-distance is and with a contig of 2^29 bases or more.
//
// --pileup [--pileup-min-count N] [--pileup-min-frac F] (mapDirectly; not in the reference; implies --edit-distance; may be combined with --paf and --bam): also
// PREFIX.pileup and PREFIX.pileup.contigs, what a column-by-column count over the PRIMARY records of PREFIX.bam gives (a read's aligned record with the largest
// field 14, the first of equals: under --all a read counts once).  PREFIX.pileup: "contigID pos ref alt count depth" (tabs; pos 0-based) for every (position,
// alt) that count >= N (an integer >= 1, default 3) and count >= F * depth (a decimal in [0, 1], default 0.2) reads support, alt one of A C G T N, - for a deleted
// base, + for an insertion behind this base; depth counts the primary alignments that span the position, deleted bases included.  PREFIX.pileup.contigs:
// "contigID length alignments covered sumDepth" for every contig with a primary alignment.  The device that mapped a batch counts its events from the traced
// alignment (mm_pileup_events, csrc/mm_pileup_core.hpp); only what differs from the reference comes to the host, where the run's pairs are merged on the device
// whenever they pass MM_PILEUP_MERGE_PAIRS; the first device finishes (mm_pileup_finish).  Both files are plain text.  Every other file of the run is the file of
// the same run without the flag.  Refused wherever --edit-distance is; the two thresholds are refused without --pileup (host/pileup_out.hpp).
//
// --vcf [--vcf-min-count N] [--vcf-min-frac F] (mapDirectly; not in the reference; implies --edit-distance; may be combined with --paf, --bam and --pileup): also
// PREFIX.vcf (VCFv4.2, sites only), the alleles of the same primary records: an SNV per mismatched base of A C G T, a deletion or an insertion per I or D run
// with an aligned base on both sides, every indel shifted left against the reference (at most 256 steps, not past the alignment's first base) so that equal
// variants of different reads count together; indels of up to 24 bases are spelt out, longer ones are <DEL> and <INS> with SVLEN and END.  INFO carries DP
// (the primary alignments that span POS) and AO (those that carry the allele); an allele is kept where AO >= N (default 3) and AO >= F * DP (default 0.2).
// The device that mapped a batch emits, shifts and counts its alleles from the traced alignment (mm_vcf_events, csrc/mm_vcf_core.hpp); the run's triples are
// merged on the device whenever they pass MM_VCF_MERGE_PAIRS; the first device finishes (mm_vcf_finish).  No genotypes, FORMAT columns, qualities or
// multi-allelic records.  Plain text; an empty run writes the header.  Every other file of the run is the file of the same run without the flag.  Refused
// wherever --edit-distance is; the two thresholds are refused without --vcf (host/vcf_out.hpp).
//
// --mods LIST [--mod-min-ml T] [--mod-min-coverage N] (mapDirectly; not in the reference; implies --edit-distance; may be combined with --paf, --bam, --pileup,
// --vcf, --consensus and --base-qualities): also PREFIX.bedmethyl, what `modkit pileup` gives over the PRIMARY records of the run: modkit's 18 tab-separated
// columns without a header, one row per reference position, strand and code of LIST with the primary alignments whose matched (=) base there carries a call.
// LIST is 1 to 4 items B+code (C+m,C+h,A+a,C+21839).  The calls come from the MM/ML tags of an unaligned BAM query (SAM tags specification, "Base
// modifications"; host/mods_out.hpp); a FASTA/FASTQ query and a BAM without the tags give an empty file and an INFO line.  The tags' skip lists become a
// (who, prob) plane beside the read's bases on the device (mm_seqset_add_mods), mm_mod_events walks the batch's one alignment call, the run's pairs are merged
// whenever they pass MM_MODS_MERGE_PAIRS and the first device finishes (mm_mod_finish).  A call whose probability byte is below T (0..255, default 204) counts
// as failed; a row is kept with N (default 1) or more valid calls.  Calls in mismatched or inserted bases count nowhere; N_delete, N_diff and N_nocall are
// written 0; --min-base-quality does not touch the counts.  Every other file of the run is the file of the same run without the flag.  Refused wherever
// --edit-distance is; the two thresholds are refused without --mods.
//
// --mod-motifs M1,M2,... [--mod-motif-min-frac F] [--mod-motif-combine-strands] (mapDirectly with --mods; not in the reference): also PREFIX.motifs.bedmethyl and
// PREFIX.motifs.tsv, what `modkit pileup --motif` and a per-contig tally of it give: which sequence motifs of which contig are methylated, and at what fraction
// of their occurrences.  An item is MOTIF:OFFSET, 1 to 32 IUPAC letters and the 0-based place of the modified base (GATC:1, CCWGG:1, CG:0), 1 to 8 of them.
// After the last batch of a query file the first device scans the packed reference for the motifs' occurrences on both strands (mm_mod_motifs: a streaming
// scan over one-hot nibbles, csrc/mm_motif.hip) and joins the merged table of --mods to them: the first file has one bedMethyl row per covered occurrence and
// code with code,MOTIF,OFFSET in column 4, the second per contig with a call, motif and code the occurrences, how many are covered (--mod-min-coverage) and
// modified (N_mod >= F of the valid calls, default 0.5), their calls and the fraction, and a last row * per motif and code.  --mod-motif-combine-strands sums the
// two strands of an occurrence (CpG-style; only motifs that are their own reverse complement).  Plain text; an empty run writes the first file empty and the
// header of the second.  Every other file of the run, PREFIX.bedmethyl included, is the file of the same run without the flag.  Refused wherever --mods is, under
// its own name; all three are refused without --mods (host/motif_out.hpp).  Not provided: motif discovery, motifs longer than 32, a modified base that is an
// ambiguity letter, several offsets per item, partial motifs at contig ends, the flag outside mapDirectly.
//
// --depth [--depth-window W] [--depth-thresholds T1,T2,...] (mapDirectly; not in the reference; implies --edit-distance; may be combined with every other side
// output): also PREFIX.depth.bedgraph, PREFIX.depth.windows and PREFIX.depth.contigs, what `samtools sort` and `mosdepth` give over the PRIMARY records of
// PREFIX.bam: the maximal runs of equal depth >= 1 (contigID start end depth, no track line), every window of W bases (default 1000, the window of
// .EM.contigCoverage) of every contig with a primary alignment (contigID start end sumDepth covered meanDepth), and per such contig a line contigID length
// alignments covered sumDepth meanDepth medianDepth maxDepth breadth expectedBreadth ge<T1> ... behind a # header (breadth = covered / length; expectedBreadth =
// 1 - exp(-sumDepth / length), what a uniform spread of that depth would cover; ge<T> the positions of depth >= T, 1 to 8 ascending integers, default
// 1,5,10,30).  Depth changes only at the alignments' ends: one mm_depth_profile call per query file on the first device, after the last batch, sorts the ends
// and works in memory proportional to the alignments, never to the reference (csrc/mm_depth_core.hpp, DESIGN.md section 1, "Depth").  It shares the one
// alignment call per batch and the intervals --pileup keeps.  Plain text whatever --compress-output says; an empty run writes the first two files empty and the
// header of the third alone.  Every other file of the run is the file of the same run without the flag.  Refused wherever --edit-distance is; the two
// options are refused without --depth (host/depth_out.hpp).  Not provided: zero-depth runs, per-strand depth, a mapping-quality filter, a quality-aware
// depth, bigWig, depth from secondary mappings, the flag outside mapDirectly.
//
// --error-profile (mapDirectly; not in the reference; implies --edit-distance; may be combined with every other side output): also
// PREFIX.errorProfile.substitutions, .indels, .qualities and .contigs from the PRIMARY alignments: which base the sequencer wrote for which base of the reference
// (counted in the read's orientation), insertions and deletions by length with those that only stretch or shrink a homopolymer apart, matches, mismatches and
// inserted bases per reported base quality with the empirical error rate (the qualities come with --base-qualities; without it every base is in the row `none`),
// and per contig the exact identity summed over its alignments, the gap-compressed identity and minimum, quartiles and maximum of the per-read identities, with a
// last row * over all alignments.  The device that mapped a batch walks its alignments once (mm_errprof_events, csrc/mm_errprof_core.hpp, DESIGN.md section 1,
// "Error profile"); the run keeps 566 sums and 32 bytes per primary alignment per query file, and the first device sorts them into the rows
// (mm_errprof_finish).  Plain text whatever --compress-output says; an empty run writes the headers alone.  Every other file of the run is the file of the same
// run without the flag.  Refused wherever --edit-distance is (host/errprof_out.hpp).  Not provided: a confusion table by the reference's homopolymer length, the
// error rate along the read, per-read rows, secondary mappings, the flag outside mapDirectly.
//
// --extract-unmapped, --extract-mapped, --extract-taxa ID[,ID...], --deplete-taxa ID[,ID...] (mapDirectly; not in the reference, whose util/extractReads.pl re-reads the
// FASTQ on the host; Kraken 2's --unclassified-out / --classified-out; may be combined with each other and with every other side output; none implies
// --edit-distance): the reads themselves, one BGZF file per flag and query file beside PREFIX, in query order: PREFIX.unmapped.fq.gz (every read without a line in
// PREFIX: the reads .meta counts as too short and as not mapped), PREFIX.mapped.fq.gz (every read with a line), PREFIX.taxa.fq.gz (the mapped reads whose PRIMARY
// line, the largest printed field 14 and the first of equals, lies on a contig whose kraken:taxid is in the list) and PREFIX.depleted.fq.gz (every read the same
// list would not take, unmapped ones included: host depletion).  A list is 1 to 64 distinct IDs x?[0-9]+, exact IDs only; under either taxon flag the reference's
// header lines are scanned first and a contig without a kraken:taxid ends the run before any device work.  With --base-qualities (accepted with these flags; implied by --min-base-quality) a record is
// "@ID\nBASES\n+\nQUAL\n" with '!' on every base of a read without qualities; without it the files are FASTA, "PREFIX.*.fa.gz", ">ID\nBASES\n" unwrapped.  ID is the
// read's ID as PREFIX prints it (1 to 254 bytes), BASES the bytes the device holds: upper-cased, IUPAC letters kept, never reverse-complemented.  The context that
// mapped a batch writes and deflates the records from the batch's packed reads (mm_reads_encode, csrc/mm_reads_out_core.hpp; host/reads_out.hpp); only the IDs go up
// and only BGZF members come back.  The inflated files do not depend on batches, devices or groups; a file without a read is the 28-byte end-of-file block.  Every
// other file of the run is the file of the same run without the flags; the packed reference is dropped as ever.  Refused, under the flag's own name: outside
// mapDirectly, --hpc, --shard-index / --stream-chunks or an index that is not resident on every device, a malformed, repeated or empty list.  Not provided: selection
// by the final EM assignment, subtree expansion of an ID, header comments and MM/ML, the original letter case, uncompressed output.
//
// --base-qualities, --min-base-quality Q (mapDirectly; not in the reference; samtools mpileup's -Q): the run keeps the base qualities of its queries (the quality
// line of a FASTQ record in any of the text forms, the qual field of a BAM record; a FASTA record and a BAM record without have none) and uploads them beside
// the bases, one byte per base (mm_seqset_add_qual; a quality character outside '!'..'~' ends the run).  --bam then writes every record's QUAL (reversed for
// strand -; 0xFF for a read without); nothing else of PREFIX.bam changes.  --min-base-quality Q, an integer 0..93 that implies --base-qualities, is a floor for
// --pileup, --vcf and --consensus: a mismatched base counts iff its quality is >= Q, a deletion iff the read's bases on either side of the gap have it, an
// insertion iff all its bases have it; a read without qualities passes every floor (mm_pileup_events_q, mm_vcf_events_q).  The alignments' intervals are
// untouched: depth, DP and PREFIX.pileup.contigs stay raw, so count / depth errs low under a floor.  With Q > 0 the VCF header gains "##minBaseQuality=Q".
// --base-qualities needs --bam, --min-base-quality, --error-profile (which counts the columns per reported quality) or one of the --extract-* / --deplete-taxa
// flags, --min-base-quality one of --pileup, --vcf, --consensus; both are refused wherever --edit-distance is.
// Without the two flags every output is what it was.
//
// --hpc (mapDirectly; not in the reference; minimap2's -H): homopolymer-compressed mapping.  Every maximal run of equal bytes of the reference and
// of the reads — as hashed: upper-cased, IUPAC and N kept — becomes one byte, on the device (mm_seqset_hpc): the reference once per device behind
// its upload, every read batch on the context that maps it.  The pipeline then runs unchanged on the compressed sequences: -m, the len < w and
// len < k skips, identities, sketch sizes and mapping qualities are in COMPRESSED space.  Lengths and coordinates are reported raw: fields 2, 4, 7
// of a mapping line and .meta.unmappedReadsLengths carry raw lengths, field 8 the raw position of the first base of the run the compressed start
// fell on, field 9 that of the last base of the run the compressed end fell on (mm_mapping_to_raw, on the device behind the mapping qualities).
// -w is chosen from the raw reference size as ever; PREFIX.parameters gains the line "hpc 1".  index / mapAgainstIndex / classify refuse the flag.
//
// --lca T (classify, mapDirectly --then-classify; not in the reference; Kraken 2's --confidence): every read is also given to the deepest taxonomy
// node whose subtree holds at least T (0.51 to 1) of its posterior mass, on the device behind the final posteriors (mm_em_lca, DESIGN.md §4 "LCA
// assignment").  PREFIX.EM.reads2Taxon.lca (readID, taxonID, rank, mass) and PREFIX.EM.kreport (the six-column Kraken report) are added; every
// other output is unchanged.
//
// --genes (classify, mapDirectly --then-classify; the reference's geneLevelAnalysis.pl, its README's "COG group analysis"): which annotated genes
// the reads' best mappings overlap.  Needs DB/DB_annotations.txt and DB/DB_proteins.faa.annotated (a gene-annotated database); a missing one ends the
// run before any work.  The interval join, the per-gene median identities and the per-read de-duplicated feature counts run on the first device
// (mm_gene_overlap, DESIGN.md §4 "Gene-level analysis").  PREFIX.EM.geneLevelAnalysis (gene, locus tag, protein, product, reads, median identity) and
// PREFIX.EM.proteins.{GO,KEGG,BiGG,OG,COG} (feature, supporting reads, their share of the mapped reads) are added; every other output is unchanged.
//
// --min-identity T [--refit] (classify, mapDirectly --then-classify; the reference's util/filterLowIdentityEntities.pl, its README's "Filtering out WIMP entries
// with low median identity"): T in [0, 1] is the script's --identityThreshold.  Genomes whose best mappings have a median identity (field 13 of the mapping
// line, in percent) below 100 T are removed, on the first device (mm_ident_filter, DESIGN.md §4 "Identity filter").  PREFIX.extractedIdentities (every
// read's largest identity, ascending), PREFIX.EM-filtered (the best mapping of every read that stays), PREFIX.EM-filtered.reads2Taxon (removed reads at 0)
// and PREFIX.EM-filtered.WIMP are added; every other output is unchanged.  --refit (not in the reference) drops the removed genomes' mappings and runs the
// EM again on what is left, so that a read whose best genome went can go to its next one: PREFIX.EM-filtered.refit, .refit.reads2Taxon, .refit.WIMP.
//
// Not provided: classifyU (disabled upstream).


#include "../mm_env.hpp"
#include "cli_switches.hpp"
#include "cli_common.hpp"
#include "cli_device.hpp"
#include "query_reader.hpp"
#include "taxonomy.hpp"
#include "classify_run.hpp"
#include "map_run.hpp"
#include "huge_new.hpp"
#include <algorithm>
#include <cerrno>
#include <cstdlib>

namespace {

Options parse(int argc, char** argv) {
  static const std::map<std::string, std::string> alias{{"-r", "reference"}, {"-q", "query"}, {"-o", "output"}, {"-k", "kmer"}, {"-p", "pval"},
      {"-w", "window"}, {"-m", "minReadLen"}, {"-t", "threads"}, {"--mm", "maxmemory"}, {"--pi", "perc_identity"}, {"-i", "index"}};
  Options o;
  for (int i = 2; i < argc; ++i) {
    std::string a = argv[i];
    if (a == "--all") { o.all = true; continue; }
    if (a == "--stream-chunks") { o.stream = true; continue; }
    if (a == "--shard-index") { o.shard = true; continue; }
    if (a == "--em-host-reduce") { o.em_host = true; continue; }
    if (a == "--host-gather" || a == "--peer-gather" || a == "--full-index" || a == "--compress-output" || a == "--hpc" || a == "--edit-distance" || a == "--paf" ||
        a == "--bam" || a == "--bam-sorted" || a == "--error-profile" ||
        a == "--pileup" || a == "--vcf" || a == "--consensus" || a == "--depth" || a == "--genes" || a == "--refit" || a == "--base-qualities" ||
        a == "--mod-motif-combine-strands" || a == "--extract-unmapped" || a == "--extract-mapped") { o.v[a.substr(2)] = "1"; continue; }
    if (a == "-h" || a == "--help") {
      std::cout << "see the header of metamaps_main.cpp / the reference's README\n"
                   "  --hpc  (mapDirectly) homopolymer-compressed mapping: runs of equal bases of the reference and the reads are collapsed on the device before\n"
                   "         sketching; -m, identities and mapping qualities are in compressed space, reported lengths and coordinates are raw\n"
                   "  --edit-distance  (mapDirectly) also writes PREFIX.editDistances: readID contigID strand d first last for every line of PREFIX, the exact edit\n"
                   "         distance of the read inside the window around its mapped position and the 0-based inclusive contig coordinates of that alignment\n"
                   "         (NA NA NA beyond 1.5 (100 - pi) % of the read length); not with --hpc, --shard-index, --stream-chunks\n"
                   "  --paf  (mapDirectly) implies --edit-distance and also writes PREFIX.paf: one PAF line with NM and a cg:Z: CIGAR of = X I D runs for every aligned\n"
                   "         line of PREFIX, the alignment traced on the device; not with --hpc, --shard-index, --stream-chunks\n"
                   "  --bam  (mapDirectly) implies --edit-distance and also writes PREFIX.bam (BGZF): one BAM record with the CIGAR, NM and MD for every aligned line of\n"
                   "         PREFIX, encoded and deflated on the device; may be combined with --paf; not with --hpc, --shard-index, --stream-chunks\n"
                   "  --bam-sorted  (mapDirectly) implies --edit-distance and also writes PREFIX.sorted.bam, the records of PREFIX.bam in ascending (contig, position, place in\n"
                   "         PREFIX.bam), merged on the device into members of 65 280 bytes, and PREFIX.sorted.bam.bai; with or without --bam; contigs below 2^29 bases;\n"
                   "         not with --hpc, --shard-index, --stream-chunks\n"
                   "  --pileup [--pileup-min-count N] [--pileup-min-frac F]  (mapDirectly) implies --edit-distance and also writes PREFIX.pileup (contigID pos ref alt count depth for\n"
                   "         every difference from the reference that at least N (default 3) primary alignments and F (default 0.2) of the depth support; alt - is a deleted\n"
                   "         base, + an insertion behind the base) and PREFIX.pileup.contigs (contigID length alignments covered sumDepth), counted on the device; may be\n"
                   "         combined with --paf and --bam; not with --hpc, --shard-index, --stream-chunks\n"
                   "  --vcf [--vcf-min-count N] [--vcf-min-frac F]  (mapDirectly) implies --edit-distance and also writes PREFIX.vcf (VCFv4.2, sites only): SNVs, deletions and\n"
                   "         insertions of the primary alignments, indels left-aligned on the device so that equal variants count together, with DP and AO; kept where at least N\n"
                   "         (default 3) alignments and F (default 0.2) of the depth carry the allele; may be combined with --paf, --bam and --pileup; not with --hpc,\n"
                   "         --shard-index, --stream-chunks\n"
                   "  --consensus [--consensus-min-depth D] [--consensus-min-frac F] [--consensus-min-called C]  (mapDirectly) implies --edit-distance and also writes\n"
                   "         PREFIX.consensus.fa, the sequence of the strain the reads come from (per contig the majority alleles of --vcf's table applied on the device where at\n"
                   "         least D (default 3) primary alignments span a position and F (default 0.5) of them carry the allele, N below D; contigs with at least C (default 0)\n"
                   "         of their length spanned), and PREFIX.consensus.tsv (per-contig counters); may be combined with --vcf, --paf, --bam and --pileup; not with --hpc,\n"
                   "         --shard-index, --stream-chunks\n"
                   "  --base-qualities  (mapDirectly, with --bam, --min-base-quality or --error-profile) the queries' base qualities (FASTQ, BAM) go to the device beside the bases;\n"
                   "         PREFIX.bam carries them in QUAL (0xFF for a read without); not with --hpc, --shard-index, --stream-chunks\n"
                   "  --min-base-quality Q  (mapDirectly, with --pileup, --vcf or --consensus) Q in [0, 93], implies --base-qualities: a mismatch counts only where its\n"
                   "         base has quality >= Q, a deletion where the read's bases on both sides of it have, an insertion where all its bases have; DP and depth stay raw\n"
                   "  --mods LIST [--mod-min-ml T] [--mod-min-coverage N]  (mapDirectly, BAM queries with MM/ML tags) implies --edit-distance and also writes PREFIX.bedmethyl\n"
                   "         (modkit's 18 columns, no header): per reference position and strand the primary alignments whose matched base carries a modified, canonical,\n"
                   "         other or failed call of each code of LIST (1 to 4 items like C+m,C+h,A+a,C+21839), counted on the device; a call fails below the ML byte T\n"
                   "         (default 204), a row needs N (default 1) valid calls; may be combined with the other outputs; not with --hpc, --shard-index, --stream-chunks\n"
                   "  --mod-motifs M1,M2,... [--mod-motif-min-frac F] [--mod-motif-combine-strands]  (mapDirectly, with --mods) also writes PREFIX.motifs.bedmethyl (a bedMethyl row\n"
                   "         per covered occurrence of a motif and code, code,MOTIF,OFFSET in column 4) and PREFIX.motifs.tsv (per contig, motif and code: occurrences, covered,\n"
                   "         modified where N_mod >= F (default 0.5) of the valid calls, and the fraction); items MOTIF:OFFSET like GATC:1,CCWGG:1,CG:0, scanned on the device\n"
                   "  --depth [--depth-window W] [--depth-thresholds T1,T2,...]  (mapDirectly) implies --edit-distance and also writes PREFIX.depth.bedgraph (contigID start end\n"
                   "         depth: the runs of equal depth >= 1 of the primary alignments), PREFIX.depth.windows (contigID start end sumDepth covered meanDepth per window of W,\n"
                   "         default 1000) and PREFIX.depth.contigs (per contig mean, median and maximal depth, breadth, the breadth a uniform spread would give and the\n"
                   "         positions of depth >= T, default 1,5,10,30), computed on the device from the alignments' ends alone; may be combined with the other outputs;\n"
                   "         not with --hpc, --shard-index, --stream-chunks\n"
                   "  --error-profile  (mapDirectly) implies --edit-distance and also writes PREFIX.errorProfile.substitutions (truth by observed base, in the read's orientation),\n"
                   "         .indels (insertions and deletions by length, those that only stretch or shrink a homopolymer apart), .qualities (matches, mismatches and inserted\n"
                   "         bases per reported base quality with the empirical error rate; needs --base-qualities, else the row `none` alone) and .contigs (per contig the\n"
                   "         exact identity of its primary alignments, gap-compressed identity and the spread across reads), counted on the device; may be combined with the\n"
                   "         other outputs; not with --hpc, --shard-index, --stream-chunks\n"
                   "  --extract-unmapped, --extract-mapped, --extract-taxa ID[,ID...], --deplete-taxa ID[,ID...]  (mapDirectly) also write the reads themselves as BGZF, in query\n"
                   "         order: PREFIX.unmapped.fq.gz (no line in PREFIX), .mapped.fq.gz (a line), .taxa.fq.gz (the primary line lies on a contig of a listed kraken:taxid) and\n"
                   "         .depleted.fq.gz (every read the list would not take); FASTQ with --base-qualities, else FASTA (.fa.gz); written and deflated on the device from the\n"
                   "         batch's packed reads; lists of 1 to 64 exact IDs; no --edit-distance implied; not with --hpc, --shard-index, --stream-chunks\n"
                   "  --lca T  (classify, mapDirectly --then-classify) T in [0.51, 1]: also assign every read to the deepest taxon that holds T of its posterior mass;\n"
                   "         adds PREFIX.EM.reads2Taxon.lca and the Kraken-style report PREFIX.EM.kreport\n"
                   "  --genes  (classify, mapDirectly --then-classify) gene-level analysis against DB_annotations.txt and DB_proteins.faa.annotated of the DB:\n"
                   "         adds PREFIX.EM.geneLevelAnalysis and PREFIX.EM.proteins.{GO,KEGG,BiGG,OG,COG}\n"
                   "  --min-identity T  (classify, mapDirectly --then-classify) T in [0, 1]: genomes whose best mappings have a median identity below T are removed and\n"
                   "         their reads set to unclassified; adds PREFIX.extractedIdentities and PREFIX.EM-filtered{,.reads2Taxon,.WIMP}\n"
                   "  --refit  (with --min-identity) also runs the EM again without the removed genomes' mappings; adds PREFIX.EM-filtered.refit{,.reads2Taxon,.WIMP}\n";
      exit(0);
    }
    std::string key = alias.count(a) ? alias.at(a) : (a.rfind("--", 0) == 0 ? a.substr(2) : "");
    if (key.empty() || i + 1 >= argc) die("Unknown or incomplete option " + a);
    o.v[key] = argv[++i];
  }
  return o;
}

// --bootstrap B [--bootstrap-seed S]: validated here (BootOpts, cli_common.hpp)
BootOpts boot_options(const Options& o) {
  BootOpts b;
  if (o.v.count("bootstrap")) {
    const std::string& v = o.v.at("bootstrap");
    const IntegerValue x = integer_value(v, 6);
    if (!x.ok || x.value < 2 || x.value > 100000) die("--bootstrap takes an integer from 2 to 100000, not '" + v + "'");
    b.B = (int)x.value;
  }
  if (o.v.count("bootstrap-seed")) {
    const std::string& v = o.v.at("bootstrap-seed");
    errno = 0;
    const IntegerValue x = integer_value(v, 20);                 // (twenty digits may pass 2^64: ERANGE)
    if (!x.ok || errno == ERANGE) die("--bootstrap-seed takes an unsigned 64-bit integer, not '" + v + "'");
    if (!b.B) die("--bootstrap-seed needs --bootstrap B");
    b.seed = (uint64_t)x.value;
  }
  return b;
}

// --lca T: validated here (LcaOpts, cli_common.hpp)
LcaOpts lca_options(const Options& o) {
  LcaOpts l;
  if (!o.v.count("lca")) return l;
  const std::string& v = o.v.at("lca");
  const DecimalValue x = decimal_value(v);
  if (!x.ok || !(x.value >= 0.51 && x.value <= 1.0)) die("--lca takes a decimal threshold from 0.51 to 1, not '" + v + "'");
  l.on = true; l.tau = x.value;
  return l;
}

// --genes: a bare flag (GeneOpts, cli_common.hpp)
GeneOpts gene_options(const Options& o) { GeneOpts g; g.on = o.v.count("genes") > 0; return g; }

// --min-identity T [--refit]: validated here (IdentOpts, cli_common.hpp)
IdentOpts ident_options(const Options& o) {
  IdentOpts f;
  f.refit = o.v.count("refit") > 0;
  if (!o.v.count("min-identity")) { if (f.refit) die("--refit needs --min-identity T"); return f; }
  const std::string& v = o.v.at("min-identity");
  const DecimalValue x = decimal_value(v);
  if (!x.ok || !(x.value >= 0.0 && x.value <= 1.0)) die("--min-identity takes a decimal threshold from 0 to 1, not '" + v + "'");
  f.on = true; f.T = x.value;
  return f;
}

// Everything classify and mapDirectly --then-classify take beside their files (ClassifyOpts, cli_common.hpp), each flag refused outside those two
// in the order of the flags here; both callers of classify_one parse through this
ClassifyOpts classify_options(const Options& o, const std::string& mode) {
  const bool classifies = mode == "classify" || (mode == "mapDirectly" && o.v.count("then-classify"));
  ClassifyOpts c;
  c.boot = boot_options(o);
  if (c.boot.B && !classifies) die("--bootstrap needs classify or mapDirectly --then-classify");
  c.lca = lca_options(o);
  if (c.lca.on && !classifies) die("--lca needs classify or mapDirectly --then-classify");
  c.genes = gene_options(o);
  if (c.genes.on && !classifies) die("--genes needs classify or mapDirectly --then-classify");
  if (c.genes.on && (mode == "mapDirectly" || o.v.count("DB"))) {  // (a database without gene annotations: said before any work)
    const std::string& db = mode == "classify" ? o.v.at("DB") : o.v.at("then-classify");
    struct stat probe;
    if (stat(gene::annotations_path(db).c_str(), &probe) != 0) die("--genes: please supply a gene-annotated database (file " + gene::annotations_path(db) + " not found).");
    if (stat(gene::proteins_path(db).c_str(), &probe) != 0) die("--genes: please supply a protein annotation file (file " + gene::proteins_path(db) + " not found).");
  }
  c.ident = ident_options(o);
  if ((c.ident.on || c.ident.refit) && !classifies) die("--min-identity and --refit need classify or mapDirectly --then-classify");
  if ((mode == "classify" || o.v.count("then-classify")) && o.v.count("minreads")) c.minReadsU = std::stoull(o.v.at("minreads"));
  return c;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2 || !(std::string(argv[1]) == "index" || std::string(argv[1]) == "mapDirectly" || std::string(argv[1]) == "mapAgainstIndex" ||
                    std::string(argv[1]) == "classify" || std::string(argv[1]) == "classifyU")) {
    std::cout << "\nMetaMaps (MI355X hot path)\n\n  Simultaneous metagenomic classification and mapping.\n\nUsage:\n\n  ./metamaps mapDirectly|classify|mapAgainstIndex|index\n\n";
    return 1;
  }
  const std::string mode = argv[1];
  if (mm::env_strict()) { const std::string bad = mm::env_unknown(); if (!bad.empty()) die("unknown MM_* environment switch(es): " + bad + " (MM_STRICT_ENV is set; see INTEGRATION.md)"); }
  const CliSwitches sw;                                           // the environment, read once (cli_switches.hpp)
  const Options o = parse(argc, argv);
  const ClassifyOpts copts = classify_options(o, mode);           // (validated before any work)
  if (o.v.count("compress-output") && mode != "mapDirectly" && mode != "mapAgainstIndex") die("--compress-output belongs to mapDirectly and mapAgainstIndex");
  // every output of mapDirectly: parsed once, and refused under its own flag's name outside mapDirectly, with --hpc and with a sharded or streamed index (output_plan.hpp)
  const OutputPlan plan = output_plan(o, mode);
  if (plan.reads.any() && o.v.count("reference")) check_reference_taxa(plan.reads, o.v.at("reference"));   // (a contig without a taxon: said before any device work)
  if (mode == "mapDirectly" || mode == "index" || mode == "mapAgainstIndex") return map_mode(o, mode, sw, plan);
  if (mode == "classify") {
    if (o.v.count("hpc")) die("--hpc belongs to mapDirectly: classify reads the raw coordinates a --hpc mapping reports and takes no such flag");
    if (!o.v.count("DB")) die("Provide path to DB.");
    if (!o.v.count("mappings")) die("Provide path to mappings.");
    const auto m0 = std::chrono::steady_clock::now();
    auto since = [&](const char* what) { if (sw.timing) std::cerr << "INFO, main: " << what << " at +" << std::chrono::duration<double>(std::chrono::steady_clock::now() - m0).count() << " s\n"; };
    std::vector<Dev> devs;
    for (int p : device_list(o, false)) { Dev d; d.phys = p; devs.push_back(d); }
    // the HIP runtime and the contexts (0.1 s; up to 2 s right behind a process that gave 150 GB back) come up on a thread of their own while the
    // mappings file is read and tokenised
    std::thread ctx_thread([&] {
      std::vector<int> phys; for (auto& d : devs) phys.push_back(d.phys);
      check_devices(phys);
      for (auto& d : devs) if (mm_ctx_create(d.phys, &d.ctx) != MM_OK) die("No MI355X (gfx950) device available — this build has no CPU path");
      since("contexts created");
    });
    JoinOnExit ctx_thread_guard{ctx_thread};
    const std::function<void()> need_devices = [&] {
      if (!ctx_thread.joinable()) return;
      const auto w0 = std::chrono::steady_clock::now();
      ctx_thread.join();
      if (sw.timing) std::cerr << "INFO, main: waited for the contexts " << std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count() << " s\n";
    };
    // an explicit --gpus 1 also goes through RCCL (one rank); --em-host-reduce: the ranks' sums are added on the host (test hook: ranks may share a device)
    const EmReduce reduce = o.em_host ? EmReduce::Host : ((devs.size() > 1 || o.v.count("gpus") || o.v.count("devices")) ? EmReduce::Rccl : EmReduce::None);
    const std::vector<std::string> files = split(o.v.at("mappings"), ",");
    for (size_t fi = 0; fi < files.size(); ++fi) {
      ClassifyHooks hooks{nullptr, need_devices};
      if (fi + 1 == files.size()) hooks.leave_now = [&] { since("mappings file done"); };
      classify_one(devs, reduce, files[fi], o.v.at("DB"), copts, hooks, nullptr, sw);
      need_devices();
      for (auto& d : devs) mm_comm_destroy(d.ctx);
      since("mappings file done");
    }
    if (!sw.full_teardown) finish_fast();
    for (auto& d : devs) mm_ctx_destroy(d.ctx);
    since("contexts destroyed");
    return 0;
  }
  die("sub-command '" + mode + "' is outside the accelerated hot path (SURVEY.md §2: Boost-archive index files / disabled upstream)");
}
