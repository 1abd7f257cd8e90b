// EM state resident in HBM: mappings grouped by read (E step) and indexed by taxon (M step).
#pragma once
#include "mm_common.hpp"

struct mm_mapping;
struct mm_em {
  mm_ctx* ctx = nullptr;
  int64_t n_reads = 0, n_entries = 0;
  int32_t n_taxa = 0;
  mm::DBuf<int64_t> read_off;      // [n_reads+1]
  mm::DBuf<int32_t> taxon;         // [n_entries]
  mm::DBuf<double> mapq, inv_nloc; // [n_entries]
  mm::DBuf<int64_t> tstart, perm;  // CSR by taxon: entries of taxon t are perm[tstart[t]..tstart[t+1]) in read order
  mm::DBuf<double> post, ll_read, f, partial, block_sum;
  // device-resident loop (mm_em_run): taxa with mappings on this rank, their partial sums, loop control, log-likelihood trace
  mm::DBuf<int32_t> present; int32_t n_present = -1;
  // the per-taxon sums in fixed shape: items of <= 512 consecutive entries of one taxon (one wavefront each), the items of present taxon p
  // are [pt_item[p], pt_item[p + 1]); the grid of the P1 / P2 launches and its per-workgroup log-likelihood partials
  mm::DBuf<int32_t> pt_item; mm::DBuf<int64_t> item_lo, item_hi; int32_t n_items = 0, n_wg = 0;
  mm::DBuf<double> item_sum, wg_ll;
  mm::DBuf<int32_t> eread;                                // read of every mapping
  mm::DBuf<int64_t> pos; mm::DBuf<double> post_sorted;   // pos[i]: place of entry i in taxon-sorted order (inverse of perm); the loop keeps its posteriors there
  mm::DBuf<double> local_partial, ll_trace, f_run;   // f_run: the loop's own frequencies (mm_em_iterate / mm_em_posteriors in between do not disturb mm_em_continue)
  mm::DBuf<long long> ctrl;
  // the bootstrap (mm_em_bootstrap, mm_boot.hip): index of every read among the reads with at least one mapping (-1: none), their number
  mm::DBuf<int32_t> mread; int64_t n_mapped = -1;
};

namespace mm {
void em_create(mm_ctx* ctx, int64_t n_reads, const int64_t* read_off, const int32_t* taxon, const double* mapq, const double* inv_nloc,
               int32_t n_taxa, mm_em* E);
void em_create_from_mapping(mm_ctx* ctx, const ::mm_mapping* M, const int32_t* contig_taxon, const int32_t* contig_len, int32_t n_contigs,
                            int32_t n_taxa, mm_em* E);
void em_iterate(mm_em* E, const double* f, double* f_partial, double* ll_partial);
void em_iterate_allreduce(mm_em* E, const double* f, double* f_next, double* ll);
void em_prepare(mm_em* E);
int em_run(mm_em* E, const double* f0, int max_iter, double* f_out, double* ll_trace, int ll_cap, bool* stopped);
int boot_run(mm_em* E, const double* f_start, int32_t rep0, int32_t n_rep, uint64_t seed, const uint8_t* weights, int max_iter,
             double* f_out, double* ll_out, int32_t* n_iter, int32_t* stopped);
void em_estep(mm_em* E, const double* f);
void em_posteriors(mm_em* E, const double* f, double* post, int64_t* best);
void comm_unique_id(char* id);
void comm_init(mm_ctx* ctx, const char* id, int rank, int nranks);
void comm_info(mm_ctx* ctx, int* n_ranks, int* rank);
void comm_allreduce_f64(mm_ctx* ctx, double* host, int64_t n);
void comm_destroy(mm_ctx* ctx);
}
