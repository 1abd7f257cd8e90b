"""ctypes binding of include/metamaps_hip.h (libmetamaps_hip.so).

Thin and literal: every wrapper is one C-ABI call (plus buffer allocation), so the parity tests exercise
exactly what a host program in another language would call.  There is no fallback: if the shared library
is missing, loading raises; if no gfx950 GPU is present, Context() raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libmetamaps_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "metamaps_hip.h")

COMM_ID_BYTES = 128
ERRPROF_COUNTERS, ERRPROF_COLS, ERRPROF_STATS = 566, 6, 12          # the sizes of mm_errprof_events' counters and columns and of a row of mm_errprof_finish (the header's constants)
DEPTH_STATS = 5                                                    # counters per contig of mm_depth_profile before its thresholds' (the header's counter constant)
MOTIF_SUMS = 5                                                      # sums per summary entry of mm_mod_motifs (the header's constant)
IUPAC_MASK = dict(A=1, C=2, G=4, T=8, R=5, Y=10, S=6, W=9, K=12, M=3, B=14, D=13, H=11, V=7, N=15)   # A 1, C 2, G 4, T 8 and their unions
CONS_STATS = 10                                                     # counters per contig of mm_consensus (the header's counter constant)
VCF_WINDOW = 25                                                     # reference bytes a kept allele of mm_vcf_finish carries (the header's window constant)
MM_ERR_ARG = -1
MM_ERR_LIMIT = -5
MM_ERR_DATA = -8


class MMError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"libmetamaps_hip status {status}: {msg}")
        self.status = status


SEED_STAGE_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int)


class MapParams(C.Structure):
    _fields_ = [("k", C.c_int32), ("w", C.c_int32), ("perc_identity", C.c_float), ("min_read_len", C.c_int32)]


class MapRecord(C.Structure):
    _fields_ = [("read", C.c_int32), ("ref_contig", C.c_int32), ("ref_start", C.c_int32), ("shared", C.c_int32),
                ("sketch", C.c_int32), ("strand", C.c_int32), ("mapq", C.c_double)]


RECORD_DTYPE = np.dtype([("read", "<i4"), ("ref_contig", "<i4"), ("ref_start", "<i4"), ("shared", "<i4"),
                         ("sketch", "<i4"), ("strand", "<i4"), ("mapq", "<f8")])
assert RECORD_DTYPE.itemsize == C.sizeof(MapRecord)


class MapStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_reads", "n_reads_long_enough", "n_reads_mapped", "n_mappings",
                                           "bases_long_enough", "sum_sketch", "sum_hits", "n_candidates",
                                           "sum_l2_stream_entries", "sum_l2_evals", "n_ambiguous_sketch_reads", "sum_hits_kept", "n_l2_rebuilds", "n_l2_wide_redo")] + \
               [(n, C.c_double) for n in ("ms_minimizer", "ms_sketch", "ms_probe_gather", "ms_sort_hits", "ms_l1_scan",
                                          "ms_l2", "ms_compact", "ms_total", "ms_hit_filter")] + \
               [("n_reads_giant", C.c_int64)]

    def as_dict(self):
        return {n: (int(getattr(self, n)) if t is C.c_int64 else float(getattr(self, n))) for n, t in self._fields_}


class IndexInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_contigs", "n_entries", "n_unique_hashes", "n_dup_flagged", "hbm_bytes")]


class SynthRefParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("n_species", C.c_int32), ("strains_per_species", C.c_int32),
                ("genome_len", C.c_int32), ("strain_divergence", C.c_float), ("genus_divergence", C.c_float)]


class SynthReadParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("n_reads", C.c_int64), ("read_len", C.c_int32), ("sub_rate", C.c_float),
                ("ins_rate", C.c_float), ("del_rate", C.c_float), ("frac_random", C.c_float), ("n_abundant", C.c_int32), ("read_len_min", C.c_int32)]


class SynthCommunityParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("n_genomes", C.c_int32), ("n_species", C.c_int32), ("n_genera", C.c_int32),
                ("median_len", C.c_double), ("sigma_len", C.c_double), ("min_len", C.c_int32), ("max_len", C.c_int32),
                ("strain_div_min", C.c_float), ("strain_div_max", C.c_float), ("genus_div_min", C.c_float), ("genus_div_max", C.c_float),
                ("strain_indel_events", C.c_int32), ("human_contigs", C.c_int32), ("human_bases", C.c_int64),
                ("repeat_fraction", C.c_float), ("n_fraction", C.c_float), ("n_repeat_families", C.c_int32), ("total_bases_target", C.c_int64)]


def declared_symbols(header: str = HEADER_PATH) -> list[str]:
    """Every function the public header declares (used by the CPU test that checks the exports)."""
    txt = open(header).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mm_[a-z0-9_]+)\s*\(", txt)))


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        path = os.environ.get("MM_LIB_PATH") or LIB_PATH            # (MM_LIB_PATH: an alternative build of the library, tools/ab.sh — A/B runs of two kernel variants on one box)
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} is missing — run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(path)
        vp, i32, i64, u64, f32, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_double
        P = C.POINTER
        sig = {
            "mm_abi_version": (C.c_int, []),
            "mm_ctx_release_cached": (C.c_int, [vp]),
            "mm_device_count": (C.c_int, []),
            "mm_ctx_create": (C.c_int, [C.c_int, P(vp)]),
            "mm_ctx_destroy": (None, [vp]),
            "mm_last_error": (C.c_char_p, [vp]),
            "mm_ctx_device_info": (C.c_int, [vp, C.c_char_p, C.c_size_t, P(C.c_int), P(u64), P(u64)]),
            "mm_ctx_synchronize": (C.c_int, [vp]),
            "mm_ctx_stream": (vp, [vp]),
            "mm_seqset_create": (C.c_int, [vp, P(vp)]),
            "mm_seqset_destroy": (None, [vp]),
            "mm_seqset_add": (C.c_int, [vp, C.c_char_p, i64]),
            "mm_seqset_add_view": (C.c_int, [vp, C.c_char_p, i64]),
            "mm_seqset_add_nt16": (C.c_int, [vp, C.c_char_p, i64, C.c_int]),
            "mm_seqset_add_qual": (C.c_int, [vp, C.c_char_p, i64, C.c_int]),
            "mm_seqset_has_qual": (C.c_int, [vp]),
            "mm_seqset_fetch_qual": (C.c_int, [vp, i64, vp, i64]),
            "mm_seqset_add_mods": (C.c_int, [vp, C.c_int32, vp, vp, vp, vp, vp, vp]),
            "mm_seqset_has_mods": (C.c_int, [vp]),
            "mm_seqset_fetch_mods": (C.c_int, [vp, i64, vp, vp, i64]),
            "mm_bgzf_inflate": (C.c_int, [vp, C.c_char_p, i64, vp, vp, C.c_int32, vp, i64, vp, vp]),
            "mm_bgzf_deflate_bound": (i64, [i64]),
            "mm_bgzf_deflate": (C.c_int, [vp, C.c_char_p, i64, vp, i64, P(i64), P(C.c_int32)]),
            "mm_gzip_open": (C.c_int, [vp, i64, i64, P(vp)]),
            "mm_gzip_feed": (C.c_int, [vp, C.c_char_p, i64, C.c_int, P(i64)]),
            "mm_gzip_read": (C.c_int, [vp, vp, i64, P(i64)]),
            "mm_gzip_stats": (C.c_int, [vp, P(i64), P(f64)]),
            "mm_gzip_close": (None, [vp]),
            "mm_seqset_save": (C.c_int, [vp, C.c_char_p]),
            "mm_seqset_load": (C.c_int, [vp, C.c_char_p, P(vp)]),
            "mm_seqset_upload": (C.c_int, [vp]),
            "mm_seqset_slice": (C.c_int, [vp, vp, i64, i64, P(vp)]),
            "mm_seqset_concat": (C.c_int, [vp, P(vp), C.c_int, P(vp)]),
            "mm_seqset_count": (i64, [vp]),
            "mm_seqset_total_bases": (i64, [vp]),
            "mm_seqset_lengths": (C.c_int, [vp, vp]),
            "mm_seqset_fetch": (C.c_int, [vp, i64, C.c_char_p, i64]),
            "mm_seqset_fetch_range": (C.c_int, [vp, i64, i64, C.c_void_p, i64]),
            "mm_seqset_hpc": (C.c_int, [vp, vp, P(vp), P(vp)]),
            "mm_hpc_map_to_raw": (C.c_int, [vp, vp, vp, i64, vp, vp]),
            "mm_hpc_map_lengths": (C.c_int, [vp, vp, vp]),
            "mm_hpc_map_device_bytes": (i64, [vp]),
            "mm_mapping_to_raw": (C.c_int, [vp, vp, vp, vp, i64]),
            "mm_hpc_map_destroy": (None, [vp]),
            "mm_synth_reference": (C.c_int, [vp, P(SynthRefParams), P(vp)]),
            "mm_synth_reads": (C.c_int, [vp, vp, P(SynthReadParams), P(vp), vp]),
            "mm_synth_community": (C.c_int, [vp, P(SynthCommunityParams), P(vp), vp]),
            "mm_synth_community_species": (C.c_int, [P(SynthCommunityParams), vp]),
            "mm_minimizers": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, i64]),
            "mm_index_build": (C.c_int, [vp, vp, C.c_int, C.c_int, P(vp)]),
            "mm_index_save": (C.c_int, [vp, C.c_char_p]),
            "mm_index_load": (C.c_int, [vp, C.c_char_p, P(vp)]),
            "mm_index_destroy": (None, [vp]),
            "mm_index_get_info": (C.c_int, [vp, P(IndexInfo)]),
            "mm_index_freq_hist": (C.c_int, [vp, vp, vp, i64, P(i64)]),
            "mm_freq_threshold_from_hist": (C.c_int, [vp, vp, i64, i64, C.c_int]),
            "mm_index_set_freq_threshold": (C.c_int, [vp, C.c_int]),
            "mm_index_entries": (C.c_int, [vp, vp, vp, vp, vp, i64]),
            "mm_index_dup_neighbours": (C.c_int, [vp, vp, vp, i64]),
            "mm_recommended_window": (C.c_int, [f64, C.c_int, f32, C.c_int, u64]),
            "mm_estimate_pvalue": (f64, [C.c_int, C.c_int, f32, C.c_int, u64]),
            "mm_min_hits_relaxed": (C.c_int, [C.c_int, C.c_int, f32]),
            "mm_identity": (None, [C.c_int, C.c_int, C.c_int, P(f32), P(f32)]),
            "mm_map_batch": (C.c_int, [vp, vp, vp, P(MapParams), P(vp)]),
            "mm_map_batch_phased": (C.c_int, [vp, vp, vp, P(MapParams), SEED_STAGE_CB, vp, P(vp)]),
            "mm_map_batch_reusing": (C.c_int, [vp, vp, vp, P(MapParams), vp, P(vp)]),
            "mm_sketch_batch": (C.c_int, [vp, vp, P(MapParams), P(vp)]),
            "mm_mapping_destroy": (None, [vp]),
            "mm_mapping_get_stats": (C.c_int, [vp, P(MapStats)]),
            "mm_comm_info": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
            "mm_mapping_gather": (C.c_int, [vp, C.c_int, i64, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp]),
            "mm_mapping_release_intermediates": (C.c_int, [vp]),
            "mm_mapping_fetch": (C.c_int, [vp, vp, vp, i64]),
            "mm_mapping_add_qualities": (C.c_int, [vp, vp, vp, C.c_int]),
            "mm_mapping_concat": (C.c_int, [vp, P(vp), vp, C.c_int, P(vp)]),
            "mm_mapping_keep_best": (C.c_int, [vp, vp, C.c_int]),
            "mm_mapping_from_parts": (C.c_int, [vp, i64, vp, P(MapParams), C.c_int, P(vp), P(vp), vp, P(vp)]),
            "mm_index_plan_chunks": (C.c_int, [vp, vp, u64, vp, i32, P(i32)]),
            "mm_debug_sketch": (C.c_int, [vp, vp, vp, vp, i64]),
            "mm_debug_hits": (C.c_int, [vp, vp, vp, vp, i64]),
            "mm_debug_candidates": (C.c_int, [vp, vp, vp, i64]),
            "mm_debug_l2": (C.c_int, [vp, vp, i64]),
            "mm_debug_min_hits": (C.c_int, [vp, vp]),
            "mm_debug_probed_lists": (C.c_int, [vp, vp, vp, i32]),
            "mm_em_create": (C.c_int, [vp, i64, vp, vp, vp, vp, i32, P(vp)]),
            "mm_em_create_from_mapping": (C.c_int, [vp, vp, vp, vp, i32, i32, P(vp)]),
            "mm_em_taxon_counts": (C.c_int, [vp, vp]),
            "mm_em_sizes": (C.c_int, [vp, P(i64), P(i64), P(i32)]),
            "mm_em_destroy": (None, [vp]),
            "mm_em_iterate": (C.c_int, [vp, vp, vp, P(f64)]),
            "mm_em_iterate_allreduce": (C.c_int, [vp, vp, vp, P(f64)]),
            "mm_em_posteriors": (C.c_int, [vp, vp, vp, vp]),
            "mm_em_run": (C.c_int, [vp, vp, C.c_int, vp, vp, C.c_int, P(C.c_int)]),
            "mm_em_continue": (C.c_int, [vp, C.c_int, vp, vp, C.c_int, P(C.c_int), P(C.c_int)]),
            "mm_em_bootstrap": (C.c_int, [vp, vp, i32, i32, u64, vp, C.c_int, vp, vp, vp, vp]),
            "mm_em_lca": (C.c_int, [vp, vp, i32, vp, vp, f64, vp, vp, vp]),
            "mm_gene_overlap": (C.c_int, [vp, i32, vp, vp, vp, vp, i32, vp, vp, i32, i64, vp, vp, vp, vp, vp, vp, vp, P(i64)]),
            "mm_ident_filter": (C.c_int, [vp, i64, vp, vp, vp, vp, i32, f64, vp, P(i64), P(i64), vp, vp, vp, vp, vp, vp, vp, P(i64), P(i64)]),
            "mm_edit_infix": (C.c_int, [vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
            "mm_mapping_edit_distances": (C.c_int, [vp, vp, vp, vp, f32, vp, vp, vp, i64]),
            "mm_edit_infix_align": (C.c_int, [vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]),
            "mm_mapping_align": (C.c_int, [vp, vp, vp, vp, f32, vp]),
            "mm_alignment_sizes": (C.c_int, [vp, vp, vp]),
            "mm_alignment_fetch": (C.c_int, [vp, vp, vp, vp, vp, vp]),
            "mm_alignment_destroy": (None, [vp]),
            "mm_bam_encode": (C.c_int, [vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp]),
            "mm_reads_encode": (C.c_int, [vp, vp, i64, vp, vp, vp, C.c_int, i64, vp]),
            "mm_reads_text_sizes": (C.c_int, [vp, vp, vp, vp]),
            "mm_reads_text_fetch": (C.c_int, [vp, vp]),
            "mm_reads_text_destroy": (None, [vp]),
            "mm_bam_encode_sorted": (C.c_int, [vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp]),
            "mm_bam_fetch_records": (C.c_int, [vp, vp, vp]),
            "mm_bam_sorter_create": (C.c_int, [vp, C.c_int32, vp, i64, vp]),
            "mm_bam_sorter_add_run": (C.c_int, [vp, vp, i64, i64, vp, vp, vp, vp]),
            "mm_bam_sorter_plan": (C.c_int, [vp, vp, vp]),
            "mm_bam_sorter_window": (C.c_int, [vp, i64, vp]),
            "mm_bam_sorter_index": (C.c_int, [vp, i64, vp]),
            "mm_bam_sorter_fetch": (C.c_int, [vp, vp]),
            "mm_bam_sorter_destroy": (None, [vp]),
            "mm_bam_sizes": (C.c_int, [vp, vp, vp, vp]),
            "mm_bam_fetch": (C.c_int, [vp, vp]),
            "mm_bam_destroy": (None, [vp]),
            "mm_pileup_events": (C.c_int, [vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
            "mm_pileup_events_q": (C.c_int, [vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int32, vp]),
            "mm_pileup_merge": (C.c_int, [vp, i64, vp, vp, vp]),
            "mm_pileup_sizes": (C.c_int, [vp, vp]),
            "mm_pileup_fetch": (C.c_int, [vp, vp, vp]),
            "mm_pileup_destroy": (None, [vp]),
            "mm_pileup_finish": (C.c_int, [vp, vp, i64, vp, vp, i64, vp, vp, vp, i64, f64, vp]),
            "mm_pileup_result_sizes": (C.c_int, [vp, vp, vp]),
            "mm_pileup_result_fetch_sites": (C.c_int, [vp, vp, vp, vp, vp]),
            "mm_pileup_result_fetch_contigs": (C.c_int, [vp, vp, vp, vp]),
            "mm_pileup_result_destroy": (None, [vp]),
            "mm_mod_events": (C.c_int, [vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int32, vp]),
            "mm_mod_merge": (C.c_int, [vp, i64, vp, vp, vp]),
            "mm_mod_sizes": (C.c_int, [vp, vp]),
            "mm_mod_fetch": (C.c_int, [vp, vp, vp]),
            "mm_mod_destroy": (None, [vp]),
            "mm_mod_finish": (C.c_int, [vp, vp, i64, vp, vp, C.c_int32, vp, i64, vp]),
            "mm_mod_result_sizes": (C.c_int, [vp, vp]),
            "mm_mod_result_fetch": (C.c_int, [vp, vp, vp, vp, vp, vp]),
            "mm_mod_result_destroy": (None, [vp]),
            "mm_mod_motifs": (C.c_int, [vp, vp, C.c_int32, C.c_int32, i64, vp, vp, C.c_int32, vp, C.c_int32, vp, vp, vp, i64, f64, C.c_int32, vp]),
            "mm_motif_result_sizes": (C.c_int, [vp, vp, vp]),
            "mm_motif_result_fetch_rows": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp]),
            "mm_motif_result_fetch_summary": (C.c_int, [vp, vp, vp, vp, vp]),
            "mm_motif_result_destroy": (None, [vp]),
            "mm_vcf_events": (C.c_int, [vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
            "mm_vcf_events_q": (C.c_int, [vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int32, vp]),
            "mm_vcf_merge": (C.c_int, [vp, i64, vp, vp, vp, vp]),
            "mm_vcf_sizes": (C.c_int, [vp, vp]),
            "mm_vcf_fetch": (C.c_int, [vp, vp, vp, vp]),
            "mm_vcf_destroy": (None, [vp]),
            "mm_vcf_finish": (C.c_int, [vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, i64, f64, vp]),
            "mm_vcf_result_sizes": (C.c_int, [vp, vp]),
            "mm_vcf_result_fetch": (C.c_int, [vp, vp, vp, vp, vp, vp]),
            "mm_vcf_result_destroy": (None, [vp]),
            "mm_consensus": (C.c_int, [vp, vp, C.c_int32, C.c_int32, i64, vp, vp, vp, i64, vp, vp, vp, i64, f64, f64, C.c_int32, vp]),
            "mm_consensus_sizes": (C.c_int, [vp, vp, vp, vp]),
            "mm_consensus_fetch_contigs": (C.c_int, [vp, vp, vp]),
            "mm_consensus_fetch_text": (C.c_int, [vp, vp, vp, vp]),
            "mm_consensus_destroy": (None, [vp]),
            "mm_depth_profile": (C.c_int, [vp, i64, vp, i64, vp, vp, vp, i64, C.c_int32, vp, vp]),
            "mm_depth_sizes": (C.c_int, [vp, vp, vp, vp]),
            "mm_depth_fetch_runs": (C.c_int, [vp, vp, vp, vp, vp]),
            "mm_depth_fetch_contigs": (C.c_int, [vp, vp, vp, vp]),
            "mm_depth_fetch_windows": (C.c_int, [vp, vp, vp]),
            "mm_depth_destroy": (None, [vp]),
            "mm_errprof_events": (C.c_int, [vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
            "mm_errprof_finish": (C.c_int, [vp, i64, i64, vp, vp, vp]),
            "mm_errprof_sizes": (C.c_int, [vp, vp]),
            "mm_errprof_fetch": (C.c_int, [vp, vp, vp]),
            "mm_errprof_destroy": (None, [vp]),
            "mm_comm_unique_id": (C.c_int, [C.c_char_p]),
            "mm_comm_init": (C.c_int, [vp, C.c_char_p, C.c_int, C.c_int]),
            "mm_comm_allreduce_f64": (C.c_int, [vp, vp, i64]),
            "mm_comm_share": (C.c_int, [vp, vp]),
            "mm_comm_destroy": (None, [vp]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _aligned_jobs(read, strand, contig, dist, first, op_off, ops, use=None):
    """(n, the contiguous arrays in the order of the C arguments) of a batch's aligned jobs, with `use` behind them where the call takes it"""
    cols = [np.ascontiguousarray(x, dtype=np.int32) for x in (read, strand, contig, dist)]
    cols += [np.ascontiguousarray(first, dtype=np.int64), np.ascontiguousarray(op_off, dtype=np.int64), np.ascontiguousarray(ops, dtype=np.uint32)]
    if use is not None:
        cols.append(np.ascontiguousarray(use, dtype=np.uint8))
    n = len(cols[0])
    assert all(len(x) == n for x in cols[1:5] + cols[7:]) and len(cols[5]) == n + 1
    return n, cols


def _table_rows(*words_and_counts):
    """(n, the contiguous arrays) of the rows of a key table: one or two columns of key words and the counts"""
    cols = [np.ascontiguousarray(x, dtype=np.uint64) for x in words_and_counts[:-1]] + [np.ascontiguousarray(words_and_counts[-1], dtype=np.uint32)]
    assert all(len(x) == len(cols[0]) for x in cols)
    return len(cols[0]), cols


class Context:
    def __init__(self, device: int = 0):
        self.h = C.c_void_p()
        st = lib().mm_ctx_create(device, C.byref(self.h))
        if st != 0:
            raise MMError(st, "mm_ctx_create failed (no gfx950 GPU visible? this library has no CPU fallback)")

    def check(self, st: int):
        if st != 0:
            raise MMError(st, lib().mm_last_error(self.h).decode(errors="replace"))

    def close(self):
        if self.h:
            lib().mm_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def device_info(self) -> dict:
        name = C.create_string_buffer(256)
        cus = C.c_int()
        tot, free = C.c_uint64(), C.c_uint64()
        self.check(lib().mm_ctx_device_info(self.h, name, 256, C.byref(cus), C.byref(tot), C.byref(free)))
        return {"name": name.value.decode(), "cus": cus.value, "hbm_total": tot.value, "hbm_free": free.value}

    def release_cached(self):
        """cached free device blocks of this context (and the device's recycled index-scale blocks) back to the driver"""
        self.check(lib().mm_ctx_release_cached(self.h))

    def synchronize(self):
        self.check(lib().mm_ctx_synchronize(self.h))

    @property
    def stream(self) -> int:
        return lib().mm_ctx_stream(self.h) or 0

    # ---- sequences
    def _upload(self, s: "SeqSet") -> "SeqSet":
        try:
            self.check(lib().mm_seqset_upload(s.h))
        except MMError:
            s.close()
            raise
        return s

    def add_mods(self, h, groups, **over):
        """mm_seqset_add_mods for the sequence added last to the set h: groups are dicts with base ("A" "C" "G" "T"), code (-1..3), mode ("." "?" "") and
        skips and ml of equal lengths, in MM's order; over: arrays in the place of the ones made from the groups (the refusal tests)"""
        off = np.zeros(len(groups) + 1, dtype=np.int64)
        np.cumsum([len(g["skips"]) for g in groups], out=off[1:])
        a = dict(base=np.array([ord(g["base"]) for g in groups], dtype=np.uint8), code=np.array([g["code"] for g in groups], dtype=np.int8),
                 mode=np.array([ord(g["mode"]) if g["mode"] else 0 for g in groups], dtype=np.uint8), off=off,
                 skips=np.array([x for g in groups for x in g["skips"]], dtype=np.uint32), ml=np.array([x for g in groups for x in g["ml"]], dtype=np.uint8))
        a.update(over)
        assert all(len(g["skips"]) == len(g["ml"]) for g in groups)
        self.check(lib().mm_seqset_add_mods(h, int(over.get("n_groups", len(groups))), _ptr(a["base"]), _ptr(a["code"]), _ptr(a["mode"]), _ptr(a["off"]), _ptr(a["skips"]), _ptr(a["ml"])))

    def seqset(self, seqs, quals=None, qual_offset=33, mods=None) -> "SeqSet":
        """an uploaded set of ASCII sequences; quals: per sequence its quality bytes (mm_seqset_add_qual with qual_offset) or None; mods: per sequence
        its modification groups (add_mods) or None"""
        h = C.c_void_p()
        self.check(lib().mm_seqset_create(self.h, C.byref(h)))
        s = SeqSet(self, h)
        keep = [None if q is None else bytes(q) for q in (quals if quals is not None else [])]   # viewed until the upload has returned
        for i, q in enumerate(seqs):
            if isinstance(q, str):
                q = q.encode()
            q = bytes(q)
            self.check(lib().mm_seqset_add(h, q, len(q)))
            if i < len(keep) and keep[i] is not None:
                self.check(lib().mm_seqset_add_qual(h, keep[i], len(keep[i]), qual_offset))
            if mods is not None and i < len(mods) and mods[i] is not None:
                self.add_mods(h, mods[i])
        return self._upload(s)

    def seqset_nt16(self, records, quals=None, qual_offset=0, mods=None) -> "SeqSet":
        """a set of BAM-packed reads: records are (4-bit code bytes, bases, reverse) as a BAM record stores them; quals: per record its quality
        bytes in the record's order (mm_seqset_add_qual with qual_offset) or None; mods: per record its modification groups (add_mods), which
        speak of the read as sequenced, or None"""
        h = C.c_void_p()
        self.check(lib().mm_seqset_create(self.h, C.byref(h)))
        s = SeqSet(self, h)
        keep = [bytes(b) for b, _, _ in records]                   # alive until the upload has returned
        keepq = [None if q is None else bytes(q) for q in (quals if quals is not None else [])]
        for i, (b, (_, n, rev)) in enumerate(zip(keep, records)):
            self.check(lib().mm_seqset_add_nt16(h, b, n, 1 if rev else 0))
            if i < len(keepq) and keepq[i] is not None:
                self.check(lib().mm_seqset_add_qual(h, keepq[i], len(keepq[i]), qual_offset))
            if mods is not None and i < len(mods) and mods[i] is not None:
                self.add_mods(h, mods[i])
        return self._upload(s)

    def bgzf_inflate(self, blocks, out_off=None, out_cap=None):
        """BGZF blocks (bytes each, whole members) inflated on the device in one call (mm_bgzf_inflate).  Returns (out, status): `out` a
        bytearray of out_cap bytes (default: the blocks' ISIZEs back to back), status one int32 per block (0 ok, 1 deflate stream invalid,
        2 length != ISIZE, 3 CRC32 mismatch, 4 malformed header).  MM_ERR_DATA (a corrupt block) is not raised: the statuses say which."""
        blocks = [bytes(b) for b in blocks]
        n = len(blocks)
        comp = b"".join(blocks)
        comp_len = np.array([len(b) for b in blocks], dtype=np.int32)
        comp_off = np.zeros(n, dtype=np.int64)
        if n:
            comp_off[1:] = np.cumsum(comp_len[:-1], dtype=np.int64)
        if out_off is None:
            isz = np.array([int.from_bytes(b[-4:], "little") if len(b) >= 26 and int.from_bytes(b[-4:], "little") <= 65536 else 0 for b in blocks],
                           dtype=np.int64)
            out_off = np.zeros(n, dtype=np.int64)
            if n:
                out_off[1:] = np.cumsum(isz[:-1])
            if out_cap is None:
                out_cap = int(isz.sum())
        out_off = np.ascontiguousarray(out_off, dtype=np.int64)
        out = bytearray(out_cap or 0)
        obuf = (C.c_uint8 * max(1, len(out))).from_buffer(out) if out else None
        status = np.zeros(n, dtype=np.int32)
        st = lib().mm_bgzf_inflate(self.h, comp, len(comp), comp_off.ctypes.data, comp_len.ctypes.data, n,
                                   C.cast(obuf, C.c_void_p) if obuf is not None else None, len(out), out_off.ctypes.data, status.ctypes.data)
        if st not in (0, MM_ERR_DATA):
            self.check(st)
        return out, status

    def bgzf_deflate(self, data, out_cap=None):
        """data (bytes) deflated into BGZF members of 65 280 input bytes each on the device (mm_bgzf_deflate).  Returns (members back to
        back as bytes, number of members); the BGZF end-of-file block is not part of it.  out_cap: the capacity passed instead of
        mm_bgzf_deflate_bound(len(data))."""
        data = bytes(data)
        cap = lib().mm_bgzf_deflate_bound(len(data)) if out_cap is None else out_cap
        out = bytearray(max(cap, 1))
        nbytes, nblocks = C.c_int64(-1), C.c_int32(-1)
        self.check(lib().mm_bgzf_deflate(self.h, data, len(data), (C.c_uint8 * len(out)).from_buffer(out), cap, C.byref(nbytes), C.byref(nblocks)))
        return bytes(out[:nbytes.value]), nblocks.value

    def gzip_inflate(self, comp, chunk_bytes: int = 0, segment_bytes: int = 0, pieces=None):
        """A plain gzip stream (bytes) inflated on the device (mm_gzip_open / feed / read).  `pieces`: the byte counts it is fed in (the
        rest goes in the last feed).  Returns (inflated bytes, stats): stats has chunks, accepted, redone, skipped, members and the seconds
        spec, chain, resolve, total.  Corrupt data raises MMError(MM_ERR_DATA) whose message names the compressed byte offset."""
        comp = bytes(comp)
        h = C.c_void_p()
        self.check(lib().mm_gzip_open(self.h, chunk_bytes, segment_bytes, C.byref(h)))
        out = bytearray()
        try:
            cuts = list(pieces or [])
            at, avail = 0, C.c_int64()
            while True:
                n = min(cuts.pop(0), len(comp) - at) if cuts else len(comp) - at
                last = at + n >= len(comp)
                self.check(lib().mm_gzip_feed(h, comp[at:at + n], n, 1 if last else 0, C.byref(avail)))
                at += n
                if avail.value:
                    buf = bytearray(avail.value)
                    got = C.c_int64()
                    self.check(lib().mm_gzip_read(h, (C.c_uint8 * len(buf)).from_buffer(buf), len(buf), C.byref(got)))
                    out += buf[:got.value]
                if last:
                    break
            counts, secs = (C.c_int64 * 5)(), (C.c_double * 4)()
            self.check(lib().mm_gzip_stats(h, counts, secs))
        finally:
            lib().mm_gzip_close(h)
        stats = dict(zip(("chunks", "accepted", "redone", "skipped", "members"), list(counts)))
        stats.update(zip(("spec_s", "chain_s", "resolve_s", "total_s"), list(secs)))
        return bytes(out), stats

    def load_seqset(self, path: str) -> "SeqSet":
        h = C.c_void_p()
        self.check(lib().mm_seqset_load(self.h, path.encode(), C.byref(h)))
        return SeqSet(self, h)

    def synth_reference(self, **kw) -> "SeqSet":
        p = SynthRefParams(**kw)
        h = C.c_void_p()
        self.check(lib().mm_synth_reference(self.h, C.byref(p), C.byref(h)))
        return SeqSet(self, h)

    def synth_community(self, **kw):
        """(reference, contig -> genome) of the SURVEY D1 community; genome n_genomes is the human-like one"""
        p = SynthCommunityParams(**kw)
        h = C.c_void_p()
        genome = np.zeros(p.n_genomes + p.human_contigs, dtype=np.int32)
        self.check(lib().mm_synth_community(self.h, C.byref(p), C.byref(h), _ptr(genome)))
        return SeqSet(self, h), genome

    @staticmethod
    def synth_community_species(**kw) -> np.ndarray:
        """genome -> species of the community synth_community(**kw) generates"""
        p = SynthCommunityParams(**kw)
        sp = np.zeros(p.n_genomes, dtype=np.int32)
        st = lib().mm_synth_community_species(C.byref(p), _ptr(sp))
        if st != 0:
            raise MMError(st, "mm_synth_community_species: bad parameters")
        return sp

    def synth_reads(self, ref: "SeqSet", **kw):
        p = SynthReadParams(**kw)
        h = C.c_void_p()
        truth = np.zeros(p.n_reads, dtype=np.int32)
        self.check(lib().mm_synth_reads(self.h, ref.h, C.byref(p), C.byref(h), _ptr(truth)))
        return SeqSet(self, h), truth

    def minimizers(self, s: "SeqSet", k: int, w: int):
        n = s.count
        off = np.zeros(n + 1, dtype=np.int64)
        self.check(lib().mm_minimizers(self.h, s.h, k, w, _ptr(off), None, None, None, 0))
        tot = int(off[-1])
        hsh = np.zeros(tot, dtype=np.uint32)
        wp = np.zeros(tot, dtype=np.int32)
        st = np.zeros(tot, dtype=np.int32)
        self.check(lib().mm_minimizers(self.h, s.h, k, w, _ptr(off), _ptr(hsh), _ptr(wp), _ptr(st), tot))
        return off, hsh, wp, st

    def index(self, contigs: "SeqSet", k: int, w: int, auto_threshold: bool = True) -> "Index":
        h = C.c_void_p()
        self.check(lib().mm_index_build(self.h, contigs.h, k, w, C.byref(h)))
        idx = Index(self, h)
        if auto_threshold:
            counts, nh = idx.freq_hist()
            thr = lib().mm_freq_threshold_from_hist(_ptr(counts), _ptr(nh), len(counts), idx.info()["n_unique_hashes"], 2**31 - 1)
            idx.set_freq_threshold(thr)
        return idx

    def load_index(self, path: str) -> "Index":
        """the persistent device index Index.save wrote (mm_index_load): no kernel runs, the stored freqThreshold is in force"""
        h = C.c_void_p()
        self.check(lib().mm_index_load(self.h, path.encode(), C.byref(h)))
        return Index(self, h)

    def map_batch(self, idx: "Index", reads: "SeqSet", k: int, w: int, pi: float = 80.0, min_read_len: int = 1000, at_seed_stage=None, at_last_kernel=None,
                  sketch_of: "Mapping | None" = None) -> "Mapping":
        """at_seed_stage / at_last_kernel: callables run between the sketch stage and the seed stage / once K5 is enqueued (mm_map_batch_phased);
        sketch_of: a mapping of the same reads (or their sketch_batch) whose minimizers and sketches are taken instead of recomputed (mm_map_batch_reusing)"""
        p = MapParams(k, w, pi, min_read_len)
        h = C.c_void_p()
        if sketch_of is not None:
            self.check(lib().mm_map_batch_reusing(self.h, idx.h, reads.h, C.byref(p), sketch_of.h, C.byref(h)))
            return Mapping(self, h, reads.count)
        if at_seed_stage is None and at_last_kernel is None:
            self.check(lib().mm_map_batch(self.h, idx.h, reads.h, C.byref(p), C.byref(h)))
        else:
            def _stage(_user, stage):
                f = at_seed_stage if stage == 1 else at_last_kernel
                if f is not None:
                    f()
            cb = SEED_STAGE_CB(_stage)
            self.check(lib().mm_map_batch_phased(self.h, idx.h, reads.h, C.byref(p), cb, None, C.byref(h)))
        return Mapping(self, h, reads.count)

    def sketch_batch(self, reads: "SeqSet", k: int, w: int, pi: float = 80.0, min_read_len: int = 1000) -> "Mapping":
        """minimizers and sketches of the reads alone (mm_sketch_batch): a `sketch_of` for map_batch against any index"""
        p = MapParams(k, w, pi, min_read_len)
        h = C.c_void_p()
        self.check(lib().mm_sketch_batch(self.h, reads.h, C.byref(p), C.byref(h)))
        return Mapping(self, h, reads.count)

    def em(self, read_off, taxon, mapq, inv_nloc, n_taxa: int) -> "EM":
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        taxon = np.ascontiguousarray(taxon, dtype=np.int32)
        mapq = np.ascontiguousarray(mapq, dtype=np.float64)
        inv_nloc = np.ascontiguousarray(inv_nloc, dtype=np.float64)
        h = C.c_void_p()
        self.check(lib().mm_em_create(self.h, len(read_off) - 1, _ptr(read_off), _ptr(taxon), _ptr(mapq), _ptr(inv_nloc), n_taxa, C.byref(h)))
        return EM(self, h, n_taxa, len(read_off) - 1, len(taxon), n_mapped=int(np.count_nonzero(np.diff(read_off))))

    def em_from_mapping(self, mapping: "Mapping", contig_taxon, contig_len, n_taxa: int) -> "EM":
        """the EM problem of `classify` built on the device from the mapping's records (after add_qualities)"""
        contig_taxon = np.ascontiguousarray(contig_taxon, dtype=np.int32)
        contig_len = np.ascontiguousarray(contig_len, dtype=np.int32)
        h = C.c_void_p()
        self.check(lib().mm_em_create_from_mapping(self.h, mapping.h, _ptr(contig_taxon), _ptr(contig_len), len(contig_taxon), n_taxa, C.byref(h)))
        nr, ne, nt = C.c_int64(), C.c_int64(), C.c_int32()
        self.check(lib().mm_em_sizes(h, C.byref(nr), C.byref(ne), C.byref(nt)))
        return EM(self, h, n_taxa, nr.value, ne.value)

    def gene_overlap(self, contig_gene_off, gene_start, gene_stop, gene_group, n_groups: int, group_feat_off, group_feat, n_feats: int,
                     map_contig, map_start, map_stop, map_ident, want_feats: bool = True, want_annotated: bool = True):
        """which annotated genes the mappings overlap (mm_gene_overlap; classify --genes): genes of contig c are [contig_gene_off[c],
        contig_gene_off[c+1]), sorted by Start.  Returns (group_reads[n_groups], group_median[n_groups] with NaN for groups without a read,
        feat_reads[n_feats] or None, mappings on contigs with genes or None)."""
        i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        i8 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
        off, gs, ge, gg, fo, ff = i8(contig_gene_off), i4(gene_start), i4(gene_stop), i4(gene_group), i8(group_feat_off), i4(group_feat)
        mc, ms, me, mi = i4(map_contig), i4(map_start), i4(map_stop), np.ascontiguousarray(map_ident, dtype=np.float64)
        reads, median = np.zeros(n_groups, dtype=np.int64), np.zeros(n_groups, dtype=np.float64)
        feats = np.zeros(n_feats, dtype=np.int64) if want_feats else None
        on = C.c_int64(-1)
        self.check(lib().mm_gene_overlap(self.h, len(off) - 1, _ptr(off), _ptr(gs), _ptr(ge), _ptr(gg), n_groups, _ptr(fo), _ptr(ff), n_feats,
                                         len(mc), _ptr(mc), _ptr(ms), _ptr(me), _ptr(mi), _ptr(reads), _ptr(median), _ptr(feats),
                                         C.byref(on) if want_annotated else None))
        return reads, median, feats, (on.value if want_annotated else None)

    def ident_filter(self, read_off, taxon, ident, best, n_taxa: int, thr_percent: float, want_filtered: bool = True) -> dict:
        """the identity filter of an EM problem (mm_ident_filter; classify --min-identity): ident in percent, best[r] an entry of read r.  Returns a
        dict of sorted_max, n_le, taxon_reads, taxon_median (NaN for a taxon without reads), taxon_removed, read_removed and, with want_filtered,
        read_src, entry_src, read_off_out of the problem without the removed taxa."""
        off, tx = np.ascontiguousarray(read_off, dtype=np.int64), np.ascontiguousarray(taxon, dtype=np.int32)
        idn, bst = np.ascontiguousarray(ident, dtype=np.float64), np.ascontiguousarray(best, dtype=np.int64)
        nr, ne = len(off) - 1, len(tx)
        smax = np.full(nr, -1.0)
        reads, median = np.full(n_taxa, -1, dtype=np.int64), np.full(n_taxa, -1.0)
        t_rem, r_rem = np.full(n_taxa, 255, dtype=np.uint8), np.full(nr, 255, dtype=np.uint8)
        n_with, n_le, n_r, n_e = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
        rs, es, ro = (np.full(nr, -1, dtype=np.int64), np.full(ne, -1, dtype=np.int64), np.full(nr + 1, -1, dtype=np.int64)) if want_filtered else (None, None, None)
        out = dict(sorted_max=smax, taxon_reads=reads, taxon_median=median, taxon_removed=t_rem, read_removed=r_rem, read_src=rs, entry_src=es, read_off_out=ro)
        st = lib().mm_ident_filter(self.h, nr, _ptr(off), _ptr(tx), _ptr(idn), _ptr(bst), n_taxa, float(thr_percent), _ptr(smax), C.byref(n_with), C.byref(n_le),
                                   _ptr(reads), _ptr(median), _ptr(t_rem), _ptr(r_rem), _ptr(rs), _ptr(es), _ptr(ro),
                                   C.byref(n_r) if want_filtered else None, C.byref(n_e) if want_filtered else None)
        if st != 0:
            err = MMError(st, lib().mm_last_error(self.h).decode(errors="replace"))
            err.outputs = dict(out, n_with_entries=n_with.value, n_le=n_le.value, n_reads_out=n_r.value, n_entries_out=n_e.value)   # (as they were handed in)
            raise err
        out.update(sorted_max=smax[:n_with.value], n_le=n_le.value, taxon_removed=t_rem.astype(bool), read_removed=r_rem.astype(bool))
        if want_filtered:
            out.update(read_src=rs[:n_r.value], entry_src=es[:n_e.value], read_off_out=ro[:n_r.value + 1])
        return out

    def edit_infix(self, reads: "SeqSet", reference: "SeqSet", read, strand, contig, ws, we, max_dist, out=None):
        """exact edit distances of arbitrary jobs (mm_edit_infix): read[i] of `reads` on strand[i] against contig[i][ws[i], we[i]) of `reference` within
        max_dist[i].  Returns (dist, begin, end), window coordinates, half-open; dist -1: not aligned.  out: the three arrays to write into."""
        rd, sd, cg, md = (np.ascontiguousarray(x, dtype=np.int32) for x in (read, strand, contig, max_dist))
        w0, w1 = np.ascontiguousarray(ws, dtype=np.int64), np.ascontiguousarray(we, dtype=np.int64)
        n = len(rd)
        assert all(len(x) == n for x in (sd, cg, md, w0, w1))
        dist, begin, end = out if out is not None else (np.full(n, -2, dtype=np.int32), np.full(n, -2, dtype=np.int64), np.full(n, -2, dtype=np.int64))
        self.check(lib().mm_edit_infix(self.h, reads.h, reference.h, n, _ptr(rd), _ptr(sd), _ptr(cg), _ptr(w0), _ptr(w1), _ptr(md), _ptr(dist), _ptr(begin), _ptr(end)))
        return dist, begin, end

    def mapping_edit_distances(self, mapping: "Mapping", reads: "SeqSet", reference: "SeqSet", perc_identity: float, n_records: int):
        """exact edit distance and 0-based inclusive contig coordinates of every record of a mapping, in fetch order (mm_mapping_edit_distances);
        (-1, -1, -1) where a record is not aligned"""
        dist, first, last = np.full(n_records, -2, dtype=np.int32), np.full(n_records, -2, dtype=np.int64), np.full(n_records, -2, dtype=np.int64)
        self.check(lib().mm_mapping_edit_distances(self.h, mapping.h, reads.h, reference.h, float(perc_identity), _ptr(dist), _ptr(first), _ptr(last), n_records))
        return dist, first, last

    def _alignment(self, status, handle):
        """(dist, first, last, op_off, ops) of an mm_alignment, which is destroyed; `handle` is NULL after an error"""
        try:
            self.check(status)
            n, k = C.c_int64(0), C.c_int64(0)
            assert lib().mm_alignment_sizes(handle, C.byref(n), C.byref(k)) == 0
            dist, first, last = np.full(n.value, -2, dtype=np.int32), np.full(n.value, -2, dtype=np.int64), np.full(n.value, -2, dtype=np.int64)
            op_off, ops = np.zeros(n.value + 1, dtype=np.int64), np.zeros(k.value, dtype=np.uint32)
            assert lib().mm_alignment_fetch(handle, _ptr(dist), _ptr(first), _ptr(last), _ptr(op_off), _ptr(ops)) == 0
            return dist, first, last, op_off, ops
        finally:
            self.last_alignment_handle = handle.value              # (what the call left in *out: None after a refusal)
            if handle.value:
                lib().mm_alignment_destroy(handle)

    def edit_infix_align(self, reads: "SeqSet", reference: "SeqSet", read, strand, contig, ws, we, max_dist):
        """edit_infix's jobs with their base-level alignments (mm_edit_infix_align).  Returns (dist, begin, end, op_off, ops): the first three as
        edit_infix gives them; the runs of job i are ops[op_off[i]:op_off[i + 1]], each len << 4 | op with I = 1, D = 2, = = 7, X = 8."""
        rd, sd, cg, md = (np.ascontiguousarray(x, dtype=np.int32) for x in (read, strand, contig, max_dist))
        w0, w1 = np.ascontiguousarray(ws, dtype=np.int64), np.ascontiguousarray(we, dtype=np.int64)
        n = len(rd)
        assert all(len(x) == n for x in (sd, cg, md, w0, w1))
        h = C.c_void_p(0xDEAD)                                      # (the call sets it, to NULL on an error)
        st = lib().mm_edit_infix_align(self.h, reads.h, reference.h, n, _ptr(rd), _ptr(sd), _ptr(cg), _ptr(w0), _ptr(w1), _ptr(md), C.byref(h))
        return self._alignment(st, h)

    def mapping_align(self, mapping: "Mapping", reads: "SeqSet", reference: "SeqSet", perc_identity: float):
        """mapping_edit_distances with the base-level alignment of every record, in fetch order (mm_mapping_align): (dist, first, last, op_off, ops)"""
        h = C.c_void_p(0xDEAD)
        st = lib().mm_mapping_align(self.h, mapping.h, reads.h, reference.h, float(perc_identity), C.byref(h))
        return self._alignment(st, h)

    def bam_encode(self, reads: "SeqSet", reference: "SeqSet", read, strand, contig, dist, first, op_off, ops, flag, mapq, names, group_bytes=0):
        """BAM records of aligned jobs as BGZF members (mm_bam_encode).  names: one bytes object per job.  Returns (members back to back as bytes,
        number of records, raw bytes of the records)."""
        return self._bam_encode(lib().mm_bam_encode, reads, reference, read, strand, contig, dist, first, op_off, ops, flag, mapq, names, group_bytes)[:3]

    def bam_encode_sorted(self, reads: "SeqSet", reference: "SeqSet", read, strand, contig, dist, first, op_off, ops, flag, mapq, names, group_bytes=0):
        """bam_encode with the records in ascending (contig, first, job) (mm_bam_encode_sorted): the same triple"""
        return self._bam_encode(lib().mm_bam_encode_sorted, reads, reference, read, strand, contig, dist, first, op_off, ops, flag, mapq, names, group_bytes)[:3]

    def bam_records(self, reads: "SeqSet", reference: "SeqSet", sorted=False, **arrays):
        """bam_encode (sorted: bam_encode_sorted) of the arrays with the records' places (mm_bam_fetch_records): (members, job of every record in stream
        order, the records' offsets in the inflated stream, one more than records)"""
        data, _, _, job, raw_off = self._bam_encode(lib().mm_bam_encode_sorted if sorted else lib().mm_bam_encode, reads, reference, **arrays)
        return data, job, raw_off

    def _bam_encode(self, entry, reads, reference, read, strand, contig, dist, first, op_off, ops, flag, mapq, names, group_bytes=0):
        """one of the two encoders: (members, records, raw bytes, job per record, offset per record and the end)"""
        n, jobs = _aligned_jobs(read, strand, contig, dist, first, op_off, ops)
        fl, mq = np.ascontiguousarray(flag, dtype=np.uint16), np.ascontiguousarray(mapq, dtype=np.uint8)
        assert all(len(x) == n for x in (fl, mq, names))
        no = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(x) for x in names], out=no[1:])
        text = np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8).copy()
        h = C.c_void_p(0xDEAD)                                      # (the call sets it, to NULL on an error)
        st = entry(self.h, reads.h, reference.h, n, *map(_ptr, jobs), _ptr(fl), _ptr(mq), _ptr(no), _ptr(text), int(group_bytes), C.byref(h))
        try:
            self.check(st)
            nr, raw, nb = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
            assert lib().mm_bam_sizes(h, C.byref(nr), C.byref(raw), C.byref(nb)) == 0
            out = np.zeros(max(nb.value, 1), dtype=np.uint8)
            assert lib().mm_bam_fetch(h, _ptr(out)) == 0
            job, raw_off = np.full(max(nr.value, 1), -1, dtype=np.int64), np.full(nr.value + 1, -1, dtype=np.int64)
            assert lib().mm_bam_fetch_records(h, _ptr(job), _ptr(raw_off)) == 0
            return out[:nb.value].tobytes(), nr.value, raw.value, job[:nr.value], raw_off
        finally:
            self.last_bam_handle = h.value                          # (what the call left in *out: None after a refusal)
            if h.value:
                lib().mm_bam_destroy(h)

    def reads_encode(self, reads: "SeqSet", read, names, with_qual, group_bytes=0):
        """FASTQ (with_qual 1) or FASTA (0) records of the reads `read` of the set under `names`, one bytes object each, as BGZF members (mm_reads_encode).
        Returns (members back to back as bytes, number of records, raw bytes of the records)."""
        rd = np.ascontiguousarray(read, dtype=np.int32)
        n = len(rd)
        assert len(names) == n
        no = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(x) for x in names], out=no[1:])
        text = np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8).copy()
        h = C.c_void_p(0xDEAD)                                      # (the call sets it, to NULL on an error)
        st = lib().mm_reads_encode(self.h, reads.h, n, _ptr(rd), _ptr(no), _ptr(text), int(with_qual), int(group_bytes), C.byref(h))
        try:
            self.check(st)
            nr, raw, nb = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
            assert lib().mm_reads_text_sizes(h, C.byref(nr), C.byref(raw), C.byref(nb)) == 0
            out = np.zeros(max(nb.value, 1), dtype=np.uint8)
            assert lib().mm_reads_text_fetch(h, _ptr(out)) == 0
            return out[:nb.value].tobytes(), nr.value, raw.value
        finally:
            self.last_reads_text_handle = h.value                   # (what the call left in *out: None after a refusal)
            if h.value:
                lib().mm_reads_text_destroy(h)

    def _key_table(self, kind, status, handle):
        """(keys, counts) of an mm_pileup or an mm_mod, (w0, w1, counts) of an mm_vcf, which is destroyed (kind: "pileup", "mod", "vcf"); `handle` is NULL after
        an error"""
        try:
            self.check(status)
            n = C.c_int64(-1)
            assert getattr(lib(), f"mm_{kind}_sizes")(handle, C.byref(n)) == 0
            words = [np.zeros(n.value, dtype=np.uint64) for _ in range(2 if kind == "vcf" else 1)]
            counts = np.zeros(n.value, dtype=np.uint32)
            assert getattr(lib(), f"mm_{kind}_fetch")(handle, *map(_ptr, words), _ptr(counts)) == 0
            return (*words, counts)
        finally:
            setattr(self, f"last_{kind}_handle", handle.value)      # (what the call left in *out: None after a refusal)
            if handle.value:
                getattr(lib(), f"mm_{kind}_destroy")(handle)

    def pileup_events(self, reads: "SeqSet", reference: "SeqSet", read, strand, contig, dist, first, op_off, ops, use, min_base_quality=None):
        """the pileup events of the jobs with use != 0 and dist >= 0 (mm_pileup_events): (keys, counts), keys contig << 35 | pos << 3 | code unique
        and ascending, code A 0 C 1 G 2 T 3 N 4, a deleted base 5, an insertion behind the base 6.  min_base_quality: mm_pileup_events_q's floor"""
        n, jobs = _aligned_jobs(read, strand, contig, dist, first, op_off, ops, use)
        h = C.c_void_p(0xDEAD)                                      # (the call sets it, to NULL on an error)
        if min_base_quality is None:
            st = lib().mm_pileup_events(self.h, reads.h, reference.h, n, *map(_ptr, jobs), C.byref(h))
        else:
            st = lib().mm_pileup_events_q(self.h, reads.h, reference.h, n, *map(_ptr, jobs), int(min_base_quality), C.byref(h))
        return self._key_table("pileup", st, h)

    def pileup_merge(self, keys, counts):
        """any (key, count) pairs, unsorted, keys may repeat -> the table with equal keys summed (mm_pileup_merge)"""
        n, rows = _table_rows(keys, counts)
        h = C.c_void_p(0xDEAD)
        st = lib().mm_pileup_merge(self.h, n, *map(_ptr, rows), C.byref(h))
        return self._key_table("pileup", st, h)

    def pileup_finish(self, reference: "SeqSet", keys, counts, iv_contig, iv_first, iv_last, min_count=3, min_frac=0.2):
        """the kept sites of a merged table and every contig's coverage from the intervals of all contributing alignments (mm_pileup_finish): a dict with
        key, count, depth, ref_byte per kept site and alignments, covered, sum_depth per contig of the reference"""
        ks, cs = np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(counts, dtype=np.uint32)
        ic = np.ascontiguousarray(iv_contig, dtype=np.int32)
        i0, i1 = np.ascontiguousarray(iv_first, dtype=np.int64), np.ascontiguousarray(iv_last, dtype=np.int64)
        assert len(ks) == len(cs) and len(ic) == len(i0) == len(i1)
        h = C.c_void_p(0xDEAD)
        st = lib().mm_pileup_finish(self.h, reference.h, len(ks), _ptr(ks), _ptr(cs), len(ic), _ptr(ic), _ptr(i0), _ptr(i1), int(min_count), float(min_frac), C.byref(h))
        try:
            self.check(st)
            ns, nc = C.c_int64(-1), C.c_int64(-1)
            assert lib().mm_pileup_result_sizes(h, C.byref(ns), C.byref(nc)) == 0
            out = dict(key=np.zeros(ns.value, dtype=np.uint64), count=np.zeros(ns.value, dtype=np.uint32), depth=np.zeros(ns.value, dtype=np.uint32),
                       ref_byte=np.zeros(ns.value, dtype=np.uint8), alignments=np.full(nc.value, -1, dtype=np.int64), covered=np.full(nc.value, -1, dtype=np.int64),
                       sum_depth=np.full(nc.value, -1, dtype=np.int64))
            assert lib().mm_pileup_result_fetch_sites(h, _ptr(out["key"]), _ptr(out["count"]), _ptr(out["depth"]), _ptr(out["ref_byte"])) == 0
            assert lib().mm_pileup_result_fetch_contigs(h, _ptr(out["alignments"]), _ptr(out["covered"]), _ptr(out["sum_depth"])) == 0
            return out
        finally:
            self.last_pileup_handle = h.value
            if h.value:
                lib().mm_pileup_result_destroy(h)

    def mod_events(self, reads: "SeqSet", reference: "SeqSet", read, strand, contig, dist, first, op_off, ops, use, min_ml=204):
        """the modification events of the jobs with use != 0 and dist >= 0 (mm_mod_events): (keys, counts), keys contig << 36 | pos << 4 |
        (strand < 0) << 3 | class unique and ascending, class 0 canonical, 1 fail (prob < min_ml), 2 another code, 3 + code"""
        n, jobs = _aligned_jobs(read, strand, contig, dist, first, op_off, ops, use)
        h = C.c_void_p(0xDEAD)
        st = lib().mm_mod_events(self.h, reads.h, reference.h, n, *map(_ptr, jobs), int(min_ml), C.byref(h))
        return self._key_table("mod", st, h)

    def mod_merge(self, keys, counts):
        """any (key, count) pairs, unsorted, keys may repeat -> the table with equal keys summed (mm_mod_merge)"""
        n, rows = _table_rows(keys, counts)
        h = C.c_void_p(0xDEAD)
        st = lib().mm_mod_merge(self.h, n, *map(_ptr, rows), C.byref(h))
        return self._key_table("mod", st, h)

    def mod_finish(self, reference: "SeqSet", keys, counts, code_base, min_coverage=1):
        """the rows of a merged table (mm_mod_finish); code_base: the base letters of the asked codes, e.g. "CCA".  A dict of arrays: site (the
        key with the code's index in the place of the class), n_mod, n_canonical, n_other, n_fail"""
        ks, cs = np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(counts, dtype=np.uint32)
        cb = np.frombuffer(code_base.encode() if isinstance(code_base, str) else bytes(code_base), dtype=np.uint8).copy()
        h = C.c_void_p(0xDEAD)
        st = lib().mm_mod_finish(self.h, reference.h, len(ks), _ptr(ks), _ptr(cs), len(cb), _ptr(cb), int(min_coverage), C.byref(h))
        try:
            self.check(st)
            n = C.c_int64()
            assert lib().mm_mod_result_sizes(h, C.byref(n)) == 0
            out = {k: np.zeros(n.value, dtype=np.uint64) for k in ("site", "n_mod", "n_canonical", "n_other", "n_fail")}
            assert lib().mm_mod_result_fetch(h, *[_ptr(out[k]) for k in ("site", "n_mod", "n_canonical", "n_other", "n_fail")]) == 0
            return out
        finally:
            self.last_mod_handle = h.value
            if h:
                lib().mm_mod_result_destroy(h)

    def mod_motifs(self, reference: "SeqSet", contig_lo, contig_hi, keys, counts, code_base, motifs, min_coverage=1, min_frac=0.5, combine_strands=False):
        """methylation per motif over the contigs [contig_lo, contig_hi) of a merged table (mm_mod_motifs); motifs: [(letters, offset)] with IUPAC letters, or
        [(masks, offset)] with the 4-bit letter sets themselves.  A dict of arrays: the covered rows (site, motif, code, n_mod, n_canonical, n_other, n_fail)
        and the summary (s_contig, s_motif, s_code, sums with MOTIF_SUMS columns: sites, covered, modified, N_valid_cov, N_mod)"""
        ks, cs = np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(counts, dtype=np.uint32)
        cb = np.frombuffer(code_base.encode() if isinstance(code_base, str) else bytes(code_base), dtype=np.uint8).copy()
        masks = [[IUPAC_MASK.get(x, 0) for x in m] if isinstance(m, str) else [int(x) for x in m] for m, _ in motifs]
        off = np.cumsum([0] + [len(m) for m in masks]).astype(np.int32)
        mask = np.array([x for m in masks for x in m] + [0], dtype=np.uint8)
        pos = np.array([int(o) for _, o in motifs] + [0], dtype=np.int32)
        h = C.c_void_p(0xDEAD)
        st = lib().mm_mod_motifs(self.h, reference.h, int(contig_lo), int(contig_hi), len(ks), _ptr(ks), _ptr(cs), len(cb), _ptr(cb), len(motifs), _ptr(off), _ptr(mask), _ptr(pos),
                                 int(min_coverage), float(min_frac), int(bool(combine_strands)), C.byref(h))
        try:
            self.check(st)
            n, ns = C.c_int64(-1), C.c_int64(-1)
            assert lib().mm_motif_result_sizes(h, C.byref(n), C.byref(ns)) == 0
            out = {k: np.zeros(n.value, dtype=np.uint64) for k in ("site", "n_mod", "n_canonical", "n_other", "n_fail")}
            out.update({k: np.zeros(n.value, dtype=np.int32) for k in ("motif", "code")})
            out.update({k: np.zeros(ns.value, dtype=np.int32) for k in ("s_contig", "s_motif", "s_code")})
            out["sums"] = np.zeros((ns.value, MOTIF_SUMS), dtype=np.int64)
            assert lib().mm_motif_result_fetch_rows(h, *[_ptr(out[k]) for k in ("site", "motif", "code", "n_mod", "n_canonical", "n_other", "n_fail")]) == 0
            assert lib().mm_motif_result_fetch_summary(h, *[_ptr(out[k]) for k in ("s_contig", "s_motif", "s_code", "sums")]) == 0
            return out
        finally:
            self.last_motif_handle = h.value
            if h.value:
                lib().mm_motif_result_destroy(h)

    def vcf_events(self, reads: "SeqSet", reference: "SeqSet", read, strand, contig, dist, first, op_off, ops, use, min_base_quality=None):
        """the left-aligned alleles of the jobs with use != 0 and dist >= 0 (mm_vcf_events): (w0, w1, counts), keys unique and ascending by (w0, w1);
        w0 = contig << 35 | pos << 3 | code (the alt's 0-3, a deletion 5, an insertion 6), w1 = 0, the deletion's length, or the insertion's length << 48
        | its bases (2 bits each, up to 24).  min_base_quality: mm_vcf_events_q's floor"""
        n, jobs = _aligned_jobs(read, strand, contig, dist, first, op_off, ops, use)
        h = C.c_void_p(0xDEAD)                                      # (the call sets it, to NULL on an error)
        if min_base_quality is None:
            st = lib().mm_vcf_events(self.h, reads.h, reference.h, n, *map(_ptr, jobs), C.byref(h))
        else:
            st = lib().mm_vcf_events_q(self.h, reads.h, reference.h, n, *map(_ptr, jobs), int(min_base_quality), C.byref(h))
        return self._key_table("vcf", st, h)

    def vcf_merge(self, w0, w1, counts):
        """any (w0, w1, count) triples, unsorted, keys may repeat -> the table with equal keys summed (mm_vcf_merge)"""
        n, rows = _table_rows(w0, w1, counts)
        h = C.c_void_p(0xDEAD)
        st = lib().mm_vcf_merge(self.h, n, *map(_ptr, rows), C.byref(h))
        return self._key_table("vcf", st, h)

    def vcf_finish(self, reference: "SeqSet", w0, w1, counts, iv_contig, iv_first, iv_last, min_count=3, min_frac=0.2):
        """the kept alleles of a merged table, their depths from the intervals of all contributing alignments and their reference windows (mm_vcf_finish):
        a dict with w0, w1, count, depth and window (25 bytes per allele)"""
        a, b, cs = np.ascontiguousarray(w0, dtype=np.uint64), np.ascontiguousarray(w1, dtype=np.uint64), np.ascontiguousarray(counts, dtype=np.uint32)
        ic = np.ascontiguousarray(iv_contig, dtype=np.int32)
        i0, i1 = np.ascontiguousarray(iv_first, dtype=np.int64), np.ascontiguousarray(iv_last, dtype=np.int64)
        assert len(a) == len(b) == len(cs) and len(ic) == len(i0) == len(i1)
        h = C.c_void_p(0xDEAD)
        st = lib().mm_vcf_finish(self.h, reference.h, len(a), _ptr(a), _ptr(b), _ptr(cs), len(ic), _ptr(ic), _ptr(i0), _ptr(i1), int(min_count), float(min_frac), C.byref(h))
        try:
            self.check(st)
            n = C.c_int64(-1)
            assert lib().mm_vcf_result_sizes(h, C.byref(n)) == 0
            out = dict(w0=np.zeros(n.value, dtype=np.uint64), w1=np.zeros(n.value, dtype=np.uint64), count=np.zeros(n.value, dtype=np.uint32),
                       depth=np.zeros(n.value, dtype=np.uint32), window=np.full((n.value, VCF_WINDOW), 0xEE, dtype=np.uint8))
            assert lib().mm_vcf_result_fetch(h, _ptr(out["w0"]), _ptr(out["w1"]), _ptr(out["count"]), _ptr(out["depth"]), _ptr(out["window"])) == 0
            return out
        finally:
            self.last_vcf_handle = h.value
            if h.value:
                lib().mm_vcf_result_destroy(h)

    def consensus(self, reference: "SeqSet", contig_lo, contig_hi, w0, w1, counts, iv_contig, iv_first, iv_last, min_depth=3, min_frac=0.5, min_called=0.0, line_width=60):
        """the consensus of the contigs [contig_lo, contig_hi) from a merged allele table and the intervals of all contributing alignments (mm_consensus): a dict
        with contig and stats (CONS_STATS counters per contig with an interval), written (the contigs whose text is there) and text ({contig: its wrapped lines})"""
        a, b, cs = np.ascontiguousarray(w0, dtype=np.uint64), np.ascontiguousarray(w1, dtype=np.uint64), np.ascontiguousarray(counts, dtype=np.uint32)
        ic = np.ascontiguousarray(iv_contig, dtype=np.int32)
        i0, i1 = np.ascontiguousarray(iv_first, dtype=np.int64), np.ascontiguousarray(iv_last, dtype=np.int64)
        assert len(a) == len(b) == len(cs) and len(ic) == len(i0) == len(i1)
        h = C.c_void_p(0xDEAD)
        st = lib().mm_consensus(self.h, reference.h, int(contig_lo), int(contig_hi), len(a), _ptr(a), _ptr(b), _ptr(cs), len(ic), _ptr(ic), _ptr(i0), _ptr(i1), int(min_depth),
                                float(min_frac), float(min_called), int(line_width), C.byref(h))
        try:
            self.check(st)
            n, nw, nb = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
            assert lib().mm_consensus_sizes(h, C.byref(n), C.byref(nw), C.byref(nb)) == 0
            contig, stats = np.zeros(n.value, dtype=np.int32), np.zeros((n.value, CONS_STATS), dtype=np.int64)
            written, off, text = np.zeros(nw.value, dtype=np.int32), np.full(nw.value + 1, -1, dtype=np.int64), np.full(nb.value, 0xEE, dtype=np.uint8)
            assert lib().mm_consensus_fetch_contigs(h, _ptr(contig), _ptr(stats)) == 0
            assert lib().mm_consensus_fetch_text(h, _ptr(written), _ptr(off), _ptr(text)) == 0
            assert off[0] == 0 and off[-1] == nb.value
            return dict(contig=contig, stats=stats, written=written, text={int(c): text[off[j]:off[j + 1]].tobytes() for j, c in enumerate(written)})
        finally:
            self.last_cons_handle = h.value                         # (what the call left in *out: None after a refusal)
            if h.value:
                lib().mm_consensus_destroy(h)

    def depth_profile(self, contig_len, iv_contig, iv_first, iv_last, window=1000, thresholds=(1, 5, 10, 30)):
        """the depth profile of the intervals over contigs of the given lengths (mm_depth_profile): a dict with the runs (run_contig, run_start, run_end,
        run_depth), the contigs with an interval (contig, win_off, stats with DEPTH_STATS + len(thresholds) counters each) and their windows (win_sum, win_covered)"""
        cl, th = np.ascontiguousarray(contig_len, dtype=np.int64), np.ascontiguousarray(thresholds, dtype=np.int64)
        ic = np.ascontiguousarray(iv_contig, dtype=np.int32)
        i0, i1 = np.ascontiguousarray(iv_first, dtype=np.int64), np.ascontiguousarray(iv_last, dtype=np.int64)
        assert len(ic) == len(i0) == len(i1)
        h = C.c_void_p(0xDEAD)
        st = lib().mm_depth_profile(self.h, len(cl), _ptr(cl), len(ic), _ptr(ic), _ptr(i0), _ptr(i1), int(window), len(th), _ptr(th), C.byref(h))
        try:
            self.check(st)
            nr, nc, nw = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
            assert lib().mm_depth_sizes(h, C.byref(nr), C.byref(nc), C.byref(nw)) == 0
            rc, rs, re_, rd = (np.full(nr.value, -1, dtype=np.int32), np.full(nr.value, -1, dtype=np.int64), np.full(nr.value, -1, dtype=np.int64),
                               np.zeros(nr.value, dtype=np.uint32))
            contig, off, stats = np.full(nc.value, -1, dtype=np.int32), np.full(nc.value + 1, -1, dtype=np.int64), np.full((nc.value, DEPTH_STATS + len(th)), -1, dtype=np.int64)
            wsum, wcov = np.full(nw.value, -1, dtype=np.int64), np.full(nw.value, -1, dtype=np.int64)
            assert lib().mm_depth_fetch_runs(h, _ptr(rc), _ptr(rs), _ptr(re_), _ptr(rd)) == 0
            assert lib().mm_depth_fetch_contigs(h, _ptr(contig), _ptr(off), _ptr(stats)) == 0
            assert lib().mm_depth_fetch_windows(h, _ptr(wsum), _ptr(wcov)) == 0
            assert off[0] == 0 and off[-1] == nw.value
            return dict(run_contig=rc, run_start=rs, run_end=re_, run_depth=rd, contig=contig, win_off=off, stats=stats, win_sum=wsum, win_covered=wcov)
        finally:
            self.last_depth_handle = h.value                        # (what the call left in *out: None after a refusal)
            if h.value:
                lib().mm_depth_destroy(h)

    def errprof_events(self, reads: "SeqSet", reference: "SeqSet", read, strand, contig, dist, first, op_off, ops, use):
        """the error profile of the jobs with use != 0 and dist >= 0 (mm_errprof_events): (counters, cols, ident_key) with ERRPROF_COUNTERS sums in the order
        SUB[25], INDEL[kind][hp][64], QUAL[cls][95], per job eq, x, insRuns, insBases, delRuns, delBases and contig << 32 | ppm (~0 for a job that is not used)"""
        n, jobs = _aligned_jobs(read, strand, contig, dist, first, op_off, ops, use)
        counters, cols, keys = np.full(ERRPROF_COUNTERS, 0xDEAD, dtype=np.uint64), np.full((n, ERRPROF_COLS), -1, dtype=np.int32), np.full(n, 0xDEAD, dtype=np.uint64)
        self.check(lib().mm_errprof_events(self.h, reads.h, reference.h, n, *map(_ptr, jobs), _ptr(counters), _ptr(cols), _ptr(keys)))
        return counters, cols, keys

    def errprof_finish(self, n_contigs, ident_key, cols):
        """the per-contig rows of the (ident_key, cols) of a query file's alignments (mm_errprof_finish): (contig, stats) with the contigs that have an alignment,
        ascending, and ERRPROF_STATS values per listed contig, the last row over all alignments together"""
        ks, cs = np.ascontiguousarray(ident_key, dtype=np.uint64), np.ascontiguousarray(cols, dtype=np.int32).reshape(-1, ERRPROF_COLS)
        assert len(ks) == len(cs)
        h = C.c_void_p(0xDEAD)
        st = lib().mm_errprof_finish(self.h, int(n_contigs), len(ks), _ptr(ks), _ptr(cs), C.byref(h))
        try:
            self.check(st)
            nc = C.c_int64(-1)
            assert lib().mm_errprof_sizes(h, C.byref(nc)) == 0
            contig, stats = np.full(nc.value, -1, dtype=np.int32), np.full((nc.value + 1, ERRPROF_STATS), -1, dtype=np.int64)
            assert lib().mm_errprof_fetch(h, _ptr(contig), _ptr(stats)) == 0
            return contig, stats
        finally:
            self.last_errprof_handle = h.value                      # (what the call left in *out: None after a refusal)
            if h.value:
                lib().mm_errprof_destroy(h)

    # ---- communicator
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(COMM_ID_BYTES)
        st = lib().mm_comm_unique_id(buf)
        if st != 0:
            raise MMError(st, "mm_comm_unique_id failed")
        return buf.raw

    def comm_init(self, uid: bytes, rank: int, nranks: int):
        self.check(lib().mm_comm_init(self.h, uid, rank, nranks))

    def comm_share(self, owner: "Context"):
        """use the communicator of another context of the same device (collectives then go out in the caller's order)"""
        self.check(lib().mm_comm_share(self.h, owner.h))

    def comm_info(self):
        """(ranks, this rank) as RCCL reports them for the context's communicator"""
        n, r = C.c_int(), C.c_int()
        self.check(lib().mm_comm_info(self.h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def comm_allreduce(self, arr: np.ndarray):
        assert arr.dtype == np.float64 and arr.flags.c_contiguous
        self.check(lib().mm_comm_allreduce_f64(self.h, _ptr(arr), arr.size))


class SeqSet:
    def __init__(self, ctx: Context, h):
        self.ctx, self.h = ctx, h

    @property
    def count(self) -> int:
        return int(lib().mm_seqset_count(self.h))

    @property
    def total_bases(self) -> int:
        return int(lib().mm_seqset_total_bases(self.h))

    def lengths(self) -> np.ndarray:
        a = np.zeros(self.count, dtype=np.int32)
        self.ctx.check(lib().mm_seqset_lengths(self.h, _ptr(a)))
        return a

    def slice(self, first: int, count: int) -> "SeqSet":
        """sequences [first, first + count) as a set of their own (device-side copy)"""
        h = C.c_void_p()
        self.ctx.check(lib().mm_seqset_slice(self.ctx.h, self.h, first, count, C.byref(h)))
        return SeqSet(self.ctx, h)

    @staticmethod
    def concat(ctx: "Context", parts: list) -> "SeqSet":
        arr = (C.c_void_p * len(parts))(*[p.h for p in parts])
        h = C.c_void_p()
        ctx.check(lib().mm_seqset_concat(ctx.h, arr, len(parts), C.byref(h)))
        return SeqSet(ctx, h)

    def save(self, path: str):
        self.ctx.check(lib().mm_seqset_save(self.h, path.encode()))

    def hpc(self, want_map: bool = False):
        """the homopolymer-compressed set (mm_seqset_hpc), compressed on the device; with want_map: (set, HpcMap back to raw coordinates)"""
        h, m = C.c_void_p(), C.c_void_p()
        self.ctx.check(lib().mm_seqset_hpc(self.ctx.h, self.h, C.byref(h), C.byref(m) if want_map else None))
        out = SeqSet(self.ctx, h)
        return (out, HpcMap(self.ctx, m, self.count)) if want_map else out

    def fetch(self, i: int, length: int) -> bytes:
        buf = C.create_string_buffer(length + 1)
        self.ctx.check(lib().mm_seqset_fetch(self.h, i, buf, length))
        return buf.raw[:length]

    @property
    def has_qual(self) -> bool:
        return bool(lib().mm_seqset_has_qual(self.h))

    def fetch_qual(self, i: int, length: int) -> bytes:
        """the stored qualities of sequence i in read order (mm_seqset_fetch_qual): Phred bytes, 0xFF each where it has none"""
        buf = np.zeros(max(length, 1), dtype=np.uint8)
        self.ctx.check(lib().mm_seqset_fetch_qual(self.h, i, _ptr(buf), length))
        return buf[:length].tobytes()

    @property
    def has_mods(self) -> bool:
        return bool(lib().mm_seqset_has_mods(self.h))

    def fetch_mods(self, i: int, length: int):
        """(who, prob) of sequence i in read order (mm_seqset_fetch_mods): who 0 no call, 1 canonical, 2 another code, 3 + code"""
        who, prob = np.zeros(max(length, 1), dtype=np.uint8), np.zeros(max(length, 1), dtype=np.uint8)
        self.ctx.check(lib().mm_seqset_fetch_mods(self.h, i, _ptr(who), _ptr(prob), length))
        return who[:length].tobytes(), prob[:length].tobytes()

    def fetch_range(self, first: int, count: int):
        """(ASCII of sequences [first, first + count) back to back as a uint8 array, their lengths)"""
        ln = self.lengths()[first:first + count]
        buf = np.empty(int(ln.sum()), dtype=np.uint8)
        self.ctx.check(lib().mm_seqset_fetch_range(self.h, first, count, buf.ctypes.data, len(buf)))
        return buf, ln

    def close(self):
        if self.h:
            lib().mm_seqset_destroy(self.h)
            self.h = None


class HpcMap:
    """compressed -> raw coordinates of a homopolymer-compressed set (mm_hpc_map)"""
    def __init__(self, ctx: Context, h, count: int):
        self.ctx, self.h, self.count = ctx, h, count

    def to_raw(self, seq, pos):
        """(raw, rawlast) of the (sequence, compressed position) pairs (mm_hpc_map_to_raw)"""
        seq = np.ascontiguousarray(seq, dtype=np.int32)
        pos = np.ascontiguousarray(pos, dtype=np.int64)
        first = np.zeros(len(seq), dtype=np.int64)
        last = np.zeros(len(seq), dtype=np.int64)
        self.ctx.check(lib().mm_hpc_map_to_raw(self.h, _ptr(seq), _ptr(pos), len(seq), _ptr(first), _ptr(last)))
        return first, last

    def lengths(self):
        """(raw lengths, compressed lengths)"""
        raw = np.zeros(self.count, dtype=np.int32)
        comp = np.zeros(self.count, dtype=np.int32)
        self.ctx.check(lib().mm_hpc_map_lengths(self.h, _ptr(raw), _ptr(comp)))
        return raw, comp

    @property
    def device_bytes(self) -> int:
        return int(lib().mm_hpc_map_device_bytes(self.h))

    def close(self):
        if self.h:
            lib().mm_hpc_map_destroy(self.h)
            self.h = None


class BamSorter:
    """sorted runs of BAM records merged into one coordinate-sorted stream of BGZF members, and its BAI (mm_bam_sorter_*)"""
    def __init__(self, ctx: Context, ref_len, window_bytes: int = 0):
        self.ctx, self.keep = ctx, []
        rl = np.ascontiguousarray(ref_len, dtype=np.int32)
        h = C.c_void_p(0xDEAD)
        st = lib().mm_bam_sorter_create(ctx.h, len(rl), _ptr(rl), int(window_bytes), C.byref(h))
        self.h = h if st == 0 else None
        ctx.check(st)

    def add_run(self, bgzf: bytes, raw_off, ref_id, pos, end):
        """a run's members (bytes, an mmap or any buffer: not copied, kept alive here until close) and its records' offsets and keys"""
        buf = np.frombuffer(bgzf, dtype=np.uint8) if len(bgzf) else np.zeros(1, dtype=np.uint8)
        ro = np.ascontiguousarray(raw_off, dtype=np.int64)
        rf, ps, en = (np.ascontiguousarray(x, dtype=np.int32) for x in (ref_id, pos, end))
        assert len(ro) == len(rf) + 1 and len(rf) == len(ps) == len(en)
        self.keep.append(buf)
        self.ctx.check(lib().mm_bam_sorter_add_run(self.h, _ptr(buf), len(bgzf), len(rf), _ptr(ro), _ptr(rf), _ptr(ps), _ptr(en)))

    def plan(self):
        """(number of windows, bytes of the sorted stream)"""
        nw, nb = C.c_int64(-1), C.c_int64(-1)
        self.ctx.check(lib().mm_bam_sorter_plan(self.h, C.byref(nw), C.byref(nb)))
        return nw.value, nb.value

    def _product(self, n: int) -> bytes:
        out = np.zeros(max(n, 1), dtype=np.uint8)
        self.ctx.check(lib().mm_bam_sorter_fetch(self.h, _ptr(out)))
        return out[:n].tobytes()

    def window(self, w: int) -> bytes:
        """the members of window w"""
        n = C.c_int64(-1)
        self.ctx.check(lib().mm_bam_sorter_window(self.h, int(w), C.byref(n)))
        return self._product(n.value)

    def index(self, header_bytes: int) -> bytes:
        """the .bai of header members of header_bytes bytes + the windows' members + the end-of-file block"""
        n = C.c_int64(-1)
        self.ctx.check(lib().mm_bam_sorter_index(self.h, int(header_bytes), C.byref(n)))
        return self._product(n.value)

    def close(self):
        if self.h:
            lib().mm_bam_sorter_destroy(self.h)
            self.h = None
        self.keep = []


class Index:
    def __init__(self, ctx: Context, h):
        self.ctx, self.h = ctx, h
        self.freq_threshold = 2**31 - 1

    def info(self) -> dict:
        i = IndexInfo()
        self.ctx.check(lib().mm_index_get_info(self.h, C.byref(i)))
        return {n: int(getattr(i, n)) for n, _ in i._fields_}

    def save(self, path: str):
        self.ctx.check(lib().mm_index_save(self.h, path.encode()))

    def freq_hist(self):
        n = C.c_int64()
        self.ctx.check(lib().mm_index_freq_hist(self.h, None, None, 0, C.byref(n)))
        counts = np.zeros(n.value, dtype=np.int64)
        nh = np.zeros(n.value, dtype=np.int64)
        self.ctx.check(lib().mm_index_freq_hist(self.h, _ptr(counts), _ptr(nh), n.value, C.byref(n)))
        return counts, nh

    def set_freq_threshold(self, thr: int):
        self.ctx.check(lib().mm_index_set_freq_threshold(self.h, int(thr)))
        self.freq_threshold = int(thr)

    def plan_chunks(self, max_memory_bytes: int) -> list[int]:
        """first contig of every --maxmemory chunk (this index must cover the whole reference)"""
        n = C.c_int32()
        self.ctx.check(lib().mm_index_plan_chunks(self.ctx.h, self.h, int(max_memory_bytes), None, 0, C.byref(n)))
        fc = np.zeros(n.value, dtype=np.int32)
        self.ctx.check(lib().mm_index_plan_chunks(self.ctx.h, self.h, int(max_memory_bytes), _ptr(fc), n.value, C.byref(n)))
        return [int(x) for x in fc]

    def entries(self):
        n = self.info()["n_entries"]
        hsh = np.zeros(n, dtype=np.uint32)
        ct = np.zeros(n, dtype=np.int32)
        wp = np.zeros(n, dtype=np.int32)
        st = np.zeros(n, dtype=np.int32)
        self.ctx.check(lib().mm_index_entries(self.h, _ptr(hsh), _ptr(ct), _ptr(wp), _ptr(st), n))
        return hsh, ct, wp, st

    def dup_neighbours(self):
        """per entry: distance to the previous / next entry of its contig with the same hash (0 = none), as K5 reads them"""
        n = self.info()["n_entries"]
        pd = np.zeros(n, dtype=np.int32)
        nd = np.zeros(n, dtype=np.int32)
        self.ctx.check(lib().mm_index_dup_neighbours(self.h, _ptr(pd), _ptr(nd), n))
        return pd, nd

    def close(self):
        if self.h:
            lib().mm_index_destroy(self.h)
            self.h = None


class Mapping:
    def __init__(self, ctx: Context, h, n_reads: int):
        self.ctx, self.h, self.n_reads = ctx, h, n_reads

    def stats(self) -> dict:
        s = MapStats()
        self.ctx.check(lib().mm_mapping_get_stats(self.h, C.byref(s)))
        return s.as_dict()

    def add_qualities(self, k: int):
        self.ctx.check(lib().mm_mapping_add_qualities(self.ctx.h, self.h, None, k))

    def to_raw(self, ref_map: "HpcMap") -> np.ndarray:
        """records of a mapping made on compressed sequences -> raw reference coordinates (mm_mapping_to_raw, after add_qualities):
        ref_start is rewritten on the device; returns the raw end of every record"""
        off = np.empty(self.n_reads + 1, dtype=np.int64)
        self.ctx.check(lib().mm_mapping_fetch(self.h, _ptr(off), None, 0))
        end = np.zeros(int(off[-1]), dtype=np.int64)
        self.ctx.check(lib().mm_mapping_to_raw(self.ctx.h, self.h, ref_map.h, _ptr(end), len(end)))
        return end

    def release_intermediates(self):
        """frees everything but the records (minimizers, sketches, hits, candidates): what a chunk mapping keeps while the other chunks are mapped"""
        self.ctx.check(lib().mm_mapping_release_intermediates(self.h))

    def keep_best(self, k: int):
        """default (non --all) reporting: per read keep identity >= best - 1.0"""
        self.ctx.check(lib().mm_mapping_keep_best(self.ctx.h, self.h, k))

    @staticmethod
    def concat(ctx: "Context", parts: list["Mapping"], contig_base: list[int]) -> "Mapping":
        arr = (C.c_void_p * len(parts))(*[p.h for p in parts])
        base = np.asarray(contig_base, dtype=np.int32)
        out = C.c_void_p()
        ctx.check(lib().mm_mapping_concat(ctx.h, arr, _ptr(base), len(parts), C.byref(out)))
        return Mapping(ctx, out, parts[0].n_reads)

    @staticmethod
    def from_parts(ctx: "Context", read_len, parts: list, contig_base: list[int], k: int, w: int, pi: float = 80.0, min_read_len: int = 1000) -> "Mapping":
        """parts = [(offsets, records)] as returned by fetch() for index chunks mapped on other GPUs"""
        rl = np.ascontiguousarray(read_len, dtype=np.int32)
        offs = [np.ascontiguousarray(o, dtype=np.int64) for o, _ in parts]
        recs = [np.ascontiguousarray(r, dtype=RECORD_DTYPE) for _, r in parts]
        oarr = (C.c_void_p * len(parts))(*[o.ctypes.data for o in offs])
        rarr = (C.c_void_p * len(parts))(*[(r.ctypes.data if len(r) else None) for r in recs])
        base = np.asarray(contig_base, dtype=np.int32)
        mp = MapParams(k, w, pi, min_read_len)
        out = C.c_void_p()
        ctx.check(lib().mm_mapping_from_parts(ctx.h, len(rl), _ptr(rl), C.byref(mp), len(parts), oarr, rarr, _ptr(base), C.byref(out)))
        return Mapping(ctx, out, len(rl))

    @staticmethod
    def gather(ctx: "Context", owner: int, read_len, parts: list["Mapping"], chunk_id: list[int], chunk_rank: list[int], contig_base: list[int],
               k: int, w: int, pi: float = 80.0, min_read_len: int = 1000):
        """mm_mapping_gather: this rank's chunk mappings of one batch -> the merged mapping on `owner` (None on the other ranks); collective"""
        rl = np.ascontiguousarray(read_len, dtype=np.int32)
        arr = (C.c_void_p * max(len(parts), 1))(*[p.h for p in parts])
        cid = np.asarray(chunk_id, dtype=np.int32); crk = np.asarray(chunk_rank, dtype=np.int32); base = np.asarray(contig_base, dtype=np.int32)
        mp = MapParams(k, w, pi, min_read_len)
        out = C.c_void_p()
        ctx.check(lib().mm_mapping_gather(ctx.h, owner, len(rl), _ptr(rl), C.byref(mp), arr, _ptr(cid), len(parts), len(crk), _ptr(crk), _ptr(base), C.byref(out)))
        return Mapping(ctx, out, len(rl)) if out.value else None

    def fetch(self, rec_buf: np.ndarray | None = None):
        """offsets [n_reads+1] and the mm_map_record array.  `rec_buf` (RECORD_DTYPE, any capacity) lets a caller
        that maps batch after batch reuse one host buffer instead of faulting in fresh pages every time."""
        off = np.empty(self.n_reads + 1, dtype=np.int64)
        self.ctx.check(lib().mm_mapping_fetch(self.h, _ptr(off), None, 0))
        n = int(off[-1])
        rec = rec_buf[:n] if rec_buf is not None and len(rec_buf) >= n else np.empty(n, dtype=RECORD_DTYPE)
        self.ctx.check(lib().mm_mapping_fetch(self.h, _ptr(off), _ptr(rec), n))
        return off, rec

    def debug_sketch(self):
        off = np.zeros(self.n_reads + 1, dtype=np.int64)
        self.ctx.check(lib().mm_debug_sketch(self.h, _ptr(off), None, None, 0))
        h = np.zeros(int(off[-1]), dtype=np.uint32)
        s = np.zeros(int(off[-1]), dtype=np.int32)
        self.ctx.check(lib().mm_debug_sketch(self.h, _ptr(off), _ptr(h), _ptr(s), len(h)))
        return off, h, s

    def debug_hits(self):
        off = np.zeros(self.n_reads + 1, dtype=np.int64)
        self.ctx.check(lib().mm_debug_hits(self.h, _ptr(off), None, None, 0))
        c = np.zeros(int(off[-1]), dtype=np.int32)
        w = np.zeros(int(off[-1]), dtype=np.int32)
        self.ctx.check(lib().mm_debug_hits(self.h, _ptr(off), _ptr(c), _ptr(w), len(c)))
        return off, c, w

    def debug_candidates(self):
        off = np.zeros(self.n_reads + 1, dtype=np.int64)
        self.ctx.check(lib().mm_debug_candidates(self.h, _ptr(off), None, 0))
        t = np.zeros((int(off[-1]), 3), dtype=np.int32)
        self.ctx.check(lib().mm_debug_candidates(self.h, _ptr(off), _ptr(t), len(t)))
        return off, t

    def debug_l2(self, n_cand: int):
        a = np.zeros((n_cand, 6), dtype=np.int64)
        if n_cand:
            self.ctx.check(lib().mm_debug_l2(self.h, _ptr(a), n_cand))
        return a

    def debug_min_hits(self):
        a = np.zeros(self.n_reads, dtype=np.int32)
        self.ctx.check(lib().mm_debug_min_hits(self.h, _ptr(a)))
        return a

    def debug_probed_lists(self, idx: "Index", n_bins: int = 66) -> np.ndarray:
        a = np.zeros(n_bins, dtype=np.int64)
        self.ctx.check(lib().mm_debug_probed_lists(self.h, idx.h, _ptr(a), n_bins))
        return a

    def close(self):
        if self.h:
            lib().mm_mapping_destroy(self.h)
            self.h = None


class EM:
    def __init__(self, ctx: Context, h, n_taxa: int, n_reads: int, n_entries: int, n_mapped: int | None = None):
        self.ctx, self.h, self.n_taxa, self.n_reads, self.n_entries = ctx, h, n_taxa, n_reads, n_entries
        self.n_mapped = n_mapped                                   # reads with at least one mapping (the bootstrap's reads), where known

    def iterate(self, f: np.ndarray):
        f = np.ascontiguousarray(f, dtype=np.float64)
        part = np.zeros(self.n_taxa, dtype=np.float64)
        ll = C.c_double()
        self.ctx.check(lib().mm_em_iterate(self.h, _ptr(f), _ptr(part), C.byref(ll)))
        return part, ll.value

    def iterate_allreduce(self, f: np.ndarray):
        f = np.ascontiguousarray(f, dtype=np.float64)
        nxt = np.zeros(self.n_taxa, dtype=np.float64)
        ll = C.c_double()
        self.ctx.check(lib().mm_em_iterate_allreduce(self.h, _ptr(f), _ptr(nxt), C.byref(ll)))
        return nxt, ll.value

    def run(self, f0: np.ndarray, max_iter: int = 1000):
        """the whole EM loop on the device: (final f, log-likelihood of every iteration)"""
        f0 = np.ascontiguousarray(f0, dtype=np.float64)
        f = np.zeros(self.n_taxa, dtype=np.float64)
        ll = np.zeros(1024, dtype=np.float64)
        n = C.c_int()
        self.ctx.check(lib().mm_em_run(self.h, _ptr(f0), max_iter, _ptr(f), _ptr(ll), len(ll), C.byref(n)))
        return f, ll[:min(n.value, len(ll))]

    def continue_run(self, max_iter: int = 1000):
        """up to max_iter more iterations from where run() / continue_run() stopped: (f, their log-likelihoods, stop rule fired)"""
        f = np.zeros(self.n_taxa, dtype=np.float64)
        ll = np.zeros(1024, dtype=np.float64)
        n, stopped = C.c_int(), C.c_int()
        self.ctx.check(lib().mm_em_continue(self.h, max_iter, _ptr(f), _ptr(ll), len(ll), C.byref(n), C.byref(stopped)))
        return f, ll[:min(n.value, len(ll))], bool(stopped.value)

    def bootstrap(self, f_start: np.ndarray, n_rep: int, seed: int, rep0: int = 0, weights=None, max_iter: int = 10_000):
        """read-level Poisson bootstrap: replicates rep0 .. rep0 + n_rep - 1 of the weighted EM from f_start (mm_em_bootstrap).
        weights: optional uint8 [n_rep, n_mapped] instead of the generated ones.  Returns (f [n_rep, n_taxa], ll [n_rep],
        n_iter [n_rep], stopped [n_rep] bool)."""
        f_start = np.ascontiguousarray(f_start, dtype=np.float64)
        if f_start.shape != (self.n_taxa,):
            raise ValueError(f"f_start must have {self.n_taxa} values")
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.uint8)
            if weights.ndim != 2 or weights.shape[0] != n_rep or (self.n_mapped is not None and weights.shape[1] != self.n_mapped):
                raise ValueError(f"weights must be uint8 [n_rep, n_mapped] = [{n_rep}, {self.n_mapped}]")
        n = max(int(n_rep), 0)
        f = np.empty((n, self.n_taxa), dtype=np.float64)           # (empty: a refused call touches none of it)
        ll = np.zeros(n, dtype=np.float64)
        it = np.zeros(n, dtype=np.int32)
        stopped = np.zeros(n, dtype=np.int32)
        self.ctx.check(lib().mm_em_bootstrap(self.h, _ptr(f_start), int(rep0), int(n_rep), int(seed) & (2**64 - 1), _ptr(weights), int(max_iter),
                                             _ptr(f), _ptr(ll), _ptr(it), _ptr(stopped)))
        return f, ll, it, stopped.astype(bool)

    def taxon_counts(self) -> np.ndarray:
        c = np.zeros(self.n_taxa, dtype=np.int64)
        self.ctx.check(lib().mm_em_taxon_counts(self.h, _ptr(c)))
        return c

    def posteriors(self, f: np.ndarray):
        f = np.ascontiguousarray(f, dtype=np.float64)
        post = np.zeros(self.n_entries, dtype=np.float64)
        best = np.zeros(self.n_reads, dtype=np.int64)
        self.ctx.check(lib().mm_em_posteriors(self.h, _ptr(f), _ptr(post), _ptr(best)))
        return post, best

    def lca(self, f: np.ndarray, parent, taxon_node, threshold: float, want_mass: bool = True, want_direct: bool = True):
        """confidence-thresholded LCA assignment of every read for the posteriors of f (mm_em_lca).  parent: the tree (parent[v] < v,
        parent[0] == 0); taxon_node [n_taxa]: the node of every taxon.  Returns (node [n_reads] int32, -1 for a read without entries;
        mass [n_reads] or None; direct [n_nodes] int64 or None)."""
        f = np.ascontiguousarray(f, dtype=np.float64)
        parent = np.ascontiguousarray(parent, dtype=np.int32)
        taxon_node = np.ascontiguousarray(taxon_node, dtype=np.int32)
        if f.shape != (self.n_taxa,) or taxon_node.shape != (self.n_taxa,):
            raise ValueError(f"f and taxon_node must have {self.n_taxa} values")
        node = np.full(self.n_reads, -2, dtype=np.int32)
        mass = np.zeros(self.n_reads, dtype=np.float64) if want_mass else None
        direct = np.zeros(len(parent), dtype=np.int64) if want_direct else None
        self.ctx.check(lib().mm_em_lca(self.h, _ptr(f), len(parent), _ptr(parent), _ptr(taxon_node), float(threshold), _ptr(node), _ptr(mass), _ptr(direct)))
        return node, mass, direct

    def close(self):
        if self.h:
            lib().mm_em_destroy(self.h)
            self.h = None
