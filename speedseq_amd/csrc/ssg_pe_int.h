/*
 * ssg_pe_int.h -- what the translation units of libssgpu share about a call of the paired-end hot path: the host result, the result kept in
 * HBM, and the entry points of ssgpu_core.cpp that ssg_bam.cpp (k_bam.h: FASTQ text in, BAM record bytes out) builds on.  (What the stage test entries of
 * ssg_dbg.cpp need of the core on top of this -- the stage runners and their types -- is in ssg_stage_int.h.)
 */
#ifndef SSG_PE_INT_H
#define SSG_PE_INT_H
#include <vector>
#include "ssg_rt.h"
#include "ssg_types.h"
#include "ssg_index_int.h"

struct ssg_pe_result {
	int n_reads, n_batches, se = 0;      /* se: the reads are single-end (ssg_mem_process_reads): n_reads units, no pairs */
	std::vector<int64_t> req_off;        /* n_reads + 1 */
	hbuf<ssg_alnreq_t> req;              /* page-locked, recycled across calls */
	hbuf<ssg_aln_t> alns;
	std::vector<ssg_pestat_t> pes;        /* n_batches * 4 */
	uint64_t stats[8];
};

/* device-resident output of the PE stage (kept in HBM for the duplicate-marking stage / the bench / the BAM record kernel) */
struct pe_dev_t {
	dbuf<ssg_alnreq_t> req; dbuf<ssg_aln_t> alns; dbuf<int64_t> req_off; int64_t n_req;
};

/* ssgpu_core.cpp */
int ssg_need_device();
/* the whole PE hot path on device-resident inputs; `keep` != NULL leaves the records in HBM instead of downloading them into `res` */
int ssg_pe_core(const ssg_index *idx, const ssg_mem_opt_t *opt, int n_pairs, const uint8_t *d_seq, const int64_t *d_off, int max_len,
                const int32_t *d_pair_batch, int n_batches, int64_t id0, const ssg_pestat_t *pes0, ssg_pe_result *res, pe_dev_t *keep);
/* exclusive prefix sum of n int32 counts into n + 1 int64 offsets, on the device; *total = out[n] */
int ssg_dev_exclusive_scan(const int32_t *d_in, int64_t *d_out, long n, int64_t *total);
/* ssg_msw_replay.cpp: mate rescue's list logic on compact keys (k_mswkeys.h) for the pairs d_todo[0 .. *d_ntodo), n_waves wavefronts (ssg_msw_replay_waves).
 * d_tmp: ssg_msw_replay_scratch() records, d_slab: *slab_bytes bytes; d_q: the queue counter; d_jres / d_jbase: the windows' slots (k_mswlane.h).  Pairs the
 * kernel gives up go to d_left, their slot bases to d_lbase (the layout of d_jbase).  d_cnt (zeroed here): [0] pairs left over, [1] pairs decided,
 * [2 .. 7] pairs left over by reason: window without a slot, missing reverse pass, tie, head-room, list too long, error code, [8] windows of the decided pairs. */
#define SSG_MSW_NCNT 9
struct ssg_msres_t;
size_t ssg_msw_replay_scratch(long n_waves, size_t *slab_bytes);
long ssg_msw_replay_waves(unsigned int n_todo, int max_wgs);
int ssg_msw_replay(const ssg_index *idx, const ssg_mem_opt_t *opt, long n_waves, const int32_t *d_todo, const unsigned int *d_ntodo, const int64_t *d_off,
                   const int64_t *d_r2off, ssg_alnreg_t *d_regs2, int32_t *d_nreg, const int32_t *d_pb, const ssg_pestat_t *d_pes,
                   ssg_alnreg_t *d_tmp, void *d_slab, unsigned int *d_q, unsigned long long *d_cells, unsigned long long *d_nrescue,
                   const ssg_msres_t *d_jres, const int64_t *d_jbase, const uint8_t *d_fixed, int tcap, int32_t *d_left, int64_t *d_lbase, unsigned int *d_cnt);
#define SSG_MAX_READ_LEN 310   /* 2x300 with room; the kernels' column classes end at 320 (k_sw.h NS = 5, the 320-column class of ssg_k_ext_lane_dyn, SSG_S2_QWORDS) */
#endif
