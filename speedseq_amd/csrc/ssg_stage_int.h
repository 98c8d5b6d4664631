/*
 * ssg_stage_int.h -- what ssg_dbg.cpp (the stage test entries) needs of ssgpu_core.cpp: the stage runners the entries go through, the types those
 * take, the scoring limits and two small device helpers.  Declarations only, and no kernel header: a unit that includes this compiles no kernel.
 */
#ifndef SSG_STAGE_INT_H
#define SSG_STAGE_INT_H
#include <vector>
#include "ssg_rt.h"
#include "../../include/ssgpu.h"
#include "ssg_index_int.h"
#include "ssg_pe_int.h"

#define SSG_STR_(x) #x
#define SSG_STR(x) SSG_STR_(x)
/* three constants of kernel headers, under names of their own; ssgpu_core.cpp, which sees both, asserts that they agree */
#define SSG_STAGE_TWIN_GLB 32768   /* SSG_TWIN_GLB (k_extend.h): the longest reference window of a region */
#define SSG_STAGE_R2D_CLASSES 3    /* SSG_R2D_CLASSES (k_aln.h): band classes of the CIGAR stage's lane DP */
#define SSG_STAGE_SBL_MAX_SPLIT 16 /* SSG_SBL_MAX_SPLIT (k_sbl.h): the largest --maxSplitCount of the splitter test */

struct align1_dev_t {	/* device-resident result of stages 1-4 */
	dbuf<int64_t> seed_off; dbuf<ssg_alnreg_t> regs; dbuf<int32_t> n_reg;
	dbuf<uint8_t> sdp_fixed;   /* per read: its region list is a fixed point of the redundancy scan (no patch alignment was involved) */
	std::vector<int64_t> h_seed_off; int64_t tot_seeds;
};
struct r2a_lists_t { std::vector<int32_t> dp[SSG_STAGE_R2D_CLASSES], todo; };   /* what the kernels left of one call: the lane DP's lists by class, the wave kernel's list */
struct msw_stage_t { unsigned long long cells, windows, from_slots, left_windows; unsigned int listed, taken, left; };
/* The pairing stage's slices, for the pipeline (ssg_pe_core) and the test entry ssg_dbg_pair_final alike: per read a region slice with head-room for rescued
 * hits (d_r2off, t2 slots in all) and a request slice (d_reqoff, tq slots), as ssg_k_pair_caps sizes them (d_cap2, d_capq); d_pkey = the pairs' region counts,
 * d_pw = the pairs heaviest first (key: candidate regions of both ends); d_regs2 = the regions (d_regoff, d_regs, d_nreg) copied into their slices. */
struct pair_slices_t {
	dbuf<int32_t> d_cap2, d_capq, d_pkey, d_pw; dbuf<int64_t> d_r2off, d_reqoff; dbuf<ssg_alnreg_t> d_regs2; int64_t t2, tq;
};
/* the samblaster view of a call's records in HBM (k_sbl.h): per pair the offset of its SAM lines, per line the line, the request it prints, what classification
 * leaves (bits, mate line); per pair the two primaries (line index or -1), their ends and the duplicate verdict */
struct sbl_lines_t {
	int64_t n_lines = 0;
	dbuf<int64_t> line_off, line_req, prim, mate; dbuf<ssg_sbl_line_t> lines; dbuf<ssg_sbl_end_t> ends; dbuf<uint8_t> bits, dup;
};
struct reg2aln_in_t { const ssg_index_t *idx; const ssg_mem_opt_t *opt; const ssg_alnreg_t *d_regs; const uint8_t *d_seq; const int64_t *d_off; int max_len; unsigned long long *d_cnt; uint64_t *stats; };

/* ssgpu_core.cpp, where each is described */
int dev_order_desc(const int32_t *d_key, int32_t *d_order, long n);
int dev_copy_regs(int n_reads, const int64_t *d_from_off, const ssg_alnreg_t *d_from, const int32_t *d_nreg, const int64_t *d_to_off, ssg_alnreg_t *d_to);
int check_band(const ssg_mem_opt_t *opt);
int check_gap_penalties(const ssg_mem_opt_t *opt);
int check_scores(const ssg_mem_opt_t *opt, int max_len);
int run_chain(const ssg_index_view_t &ix, const ssg_mem_opt_t *opt, int n_reads, const int64_t *d_off, int max_len, const ssg_intv_t *d_intv, const int32_t *d_nintv, int cap,
              const int32_t *d_nseed, const int64_t *seed_off, ssg_seed_t *d_seeds, const int32_t *d_srid, ssg_chain_t *d_chains, int32_t *d_order, int32_t *d_kept,
              int32_t *d_cseeds, int32_t *d_nchain, const int32_t *d_work, unsigned int *d_queue, uint64_t *n_tree, int32_t *form);
int run_regions(const ssg_index_view_t &ix, const ssg_mem_opt_t *opt, int n_reads, const uint8_t *d_seq, const int64_t *d_off, int max_len, size_t ts,
                const ssg_seed_t *d_seeds_p, const ssg_chain_t *d_chains_p, const int32_t *d_order_p, const int32_t *d_cseeds_p, const int32_t *d_nchain_p,
                const int32_t *d_work_p, unsigned int *d_queue_p, align1_dev_t &o, uint64_t *cells, uint64_t *n_jobs_out, std::vector<int32_t> *todo);
int run_reg2aln(const ssg_index_view_t &ix, const ssg_mem_opt_t *opt, int64_t nreq, const ssg_alnreq_t *d_creq, const ssg_alnreg_t *d_regs, const uint8_t *d_seq, const int64_t *d_off,
                ssg_aln_t *d_alns, int32_t *d_gerr, unsigned long long *d_cnt, int max_len, r2a_lists_t *lists = 0);
int run_pestat(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_pairs, const int64_t *d_regoff, const ssg_alnreg_t *d_regs, const int32_t *d_nreg,
               const int32_t *d_pb, int n_batches, ssg_pestat_t *pes /* n_batches x 4 */);
int run_pair_final(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_pairs, int64_t id0, int64_t t2, const int64_t *d_r2off, ssg_alnreg_t *d_regs2, const int32_t *d_nreg,
                   const int32_t *d_pb, const ssg_pestat_t *d_pes, const int32_t *d_pkey, const int32_t *d_pw, int32_t *d_zbuf,
                   const int64_t *d_reqoff, ssg_alnreq_t *d_req, int32_t *d_nreq, int32_t *d_perr, unsigned int *d_q);
int run_matesw(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_pairs, const uint8_t *d_seq, const int64_t *d_off, int max_len, const int64_t *d_r2off, ssg_alnreg_t *d_regs2,
               int32_t *d_nreg, const int32_t *d_pb, const ssg_pestat_t *d_pes, const int32_t *d_pw, const uint8_t *d_fixed, int32_t *d_perr, unsigned long long *d_cnt,
               unsigned int *d_q, msw_stage_t *ms);
void msw_counts(const msw_stage_t &m, uint64_t counts[8]);   /* counts[0 .. 6] of ssg_dbg_matesw / ssg_dbg_matesw_last (include/ssgpu.h); counts[7] = 0 */
int make_pair_slices(int n_reads, const int64_t *d_regoff, const ssg_alnreg_t *d_regs, const int32_t *d_nreg, int max_matesw, pair_slices_t &s);
int run_req_tail(int n_reads, const int64_t *d_reqoff, const ssg_alnreq_t *d_req, const int32_t *d_nreq, int64_t *h_off, const reg2aln_in_t *a, pe_dev_t &t);
int records_lines(long n_pairs, const int64_t *d_req_off, const ssg_alnreq_t *d_req, const ssg_aln_t *d_alns, sbl_lines_t *R);
int records_dedup(ssg_sbl_state_t *st, long n_pairs, const ssg_sbl_end_t *d_ends, uint8_t *d_dup, uint64_t *d_sig_out);
int records_classify(long n_pairs, sbl_lines_t *R, const ssg_sbl_opt_t *o, const uint8_t *d_dup, uint64_t counts[4]);
int records_export(const sbl_lines_t *R, const ssg_aln_t *d_alns, uint64_t *d_keys, ssg_aln_t *d_recs, uint8_t *d_bits);
#endif
