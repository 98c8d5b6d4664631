/*
 * k_bam_select.h -- the records of a scanned chunk decided on the device and the kept ones compacted there (what the kernel
 * stands for in the reference: the overlap test of a region iterator, htslib hts_itr_next, and the flag / MAPQ tests of `samtools view', sam_view.c
 * process_aln).  The chunk lies in the record store, loc[] / key[] / ent[] of its n_rec records in device memory as ssg_k_bam_walk and ssg_k_bam_fields
 * (k_bam_scan.h) left them.  A kernel of a translation unit of its own (ssg_bam_select.cpp): the pinned machine code of the other kernels does not move.
 *
 * ssg_k_bam_select, a lane per record.  The lane reads the record's 36 fixed bytes at loc[i] (the walk has seen that they lie inside the stream) and takes the
 * record's end from ent[i]: the CIGAR is not walked again.  A record is kept when
 *   - it overlaps a region (no test when n_reg == 0): reg[] is sorted by (tid, beg), disjoint and not adjacent (the host checks that), so only two regions can
 *     overlap a record that none before them overlaps: the last one that begins at or before the record's pos, and its successor.  The first is found by
 *     bisection; the trip count n_steps (the smallest s with 2^s > n_reg) is the host's, the same for every lane, and a lane that has converged or has
 *     tid < 0 idles: no load is issued outside reg[0 .. n_reg).  Overlap: the same tid, pos < reg.end and rec.end > reg.beg;
 *   - and the filter program leaves 1 (kept when n_prog == 0): postfix, at most 64 operations, the same for every lane -- the program counter, the operation
 *     and its constant are wave-uniform (scalar loads), only the record's fields differ per lane, and the field of a comparison is chosen by uniform
 *     branches over registers.  The boolean stack is one 64-bit word per lane, the top in bit 0; the host has checked that no operation underflows it and
 *     that it ends one deep.
 * It runs twice, as ssg_k_bam_walk does: with base == NULL a wave ballots its kept lanes, the four popcounts of a workgroup meet in 16 bytes of LDS and their
 * sum becomes cnt[workgroup]; after an exclusive scan of the counts the same decision is taken again and a kept lane writes loc, key and ent at
 * base[workgroup] + the popcounts of the waves before its own + the kept lanes below it in the ballot: stream order is kept.  Every store is bounds-checked
 * against n_out.  Both loops have wave-uniform trip counts; nothing is indexed by a lane-variant value but the record and its region.
 */
#ifndef SSG_K_BAM_SELECT_H
#define SSG_K_BAM_SELECT_H
#include "ssg_dev.h"
#include "../../include/ssgpu.h"

#define SEL_OFF_MASK (((uint64_t)1 << 40) - 1)   /* the offset of a location (BS_OFF_MASK, k_bam_scan.h) */

SSG_DEVFN bool sel_overlaps(const ssg_bam_region_t &r, int32_t tid, int32_t pos, int32_t end) { return r.tid == tid && pos < r.end && end > r.beg; }

SSG_DEVFN bool sel_keep(const uint8_t *chunk, uint64_t off, int32_t end, bool act, const ssg_bam_region_t *reg, int32_t n_reg, int32_t n_steps, const ssg_bam_fop_t *prog, int32_t n_prog)
{
	uint32_t x[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
	if (act) memcpy(x, chunk + off, 36);   /* block_size, tid, pos, bin_mq_nl, flag_nc, l_seq, mtid, mpos, isize */
	const int32_t tid = (int32_t)x[1], pos = (int32_t)x[2], mapq = (int32_t)(x[3] >> 8 & 0xffu), flag = (int32_t)(x[4] >> 16), l_seq = (int32_t)x[5], mtid = (int32_t)x[6], isize = (int32_t)x[8];
	bool in = n_reg == 0;
	if (n_reg > 0) {
		const bool q = act && tid >= 0;
		int32_t lo = 0, hi = n_reg;   /* lo becomes the number of regions that begin at or before (tid, pos) */
		for (int32_t s = 0; s < n_steps; ++s) {
			if (q && lo < hi) {
				const int32_t mid = (int32_t)(((uint32_t)lo + (uint32_t)hi) >> 1);
				const int32_t rt = reg[mid].tid, rb = reg[mid].beg;
				if (rt < tid || (rt == tid && rb <= pos)) lo = mid + 1; else hi = mid;
			}
		}
		if (q) {
			if (lo > 0) in = sel_overlaps(reg[lo - 1], tid, pos, end);
			if (!in && lo < n_reg) in = sel_overlaps(reg[lo], tid, pos, end);
		}
	}
	uint64_t stk = n_prog == 0 ? 1u : 0u;
	for (int32_t pc = 0; pc < n_prog; ++pc) {
		const uint32_t op = prog[pc].op, arg = prog[pc].arg; const int32_t c = prog[pc].value;
		if (op == SSG_FOP_AND) { const uint64_t b = stk & 1u; stk >>= 1; stk &= ~(uint64_t)1 | b; }
		else if (op == SSG_FOP_OR) { const uint64_t b = stk & 1u; stk >>= 1; stk |= b; }
		else if (op == SSG_FOP_NOT) stk ^= 1u;
		else if (op == SSG_FOP_FLAG) stk = stk << 1 | ((flag & c) != 0 ? 1u : 0u);
		else {
			int32_t v = mapq;
			if (arg == SSG_FLD_REF_ID) v = tid; else if (arg == SSG_FLD_MATE_REF_ID) v = mtid; else if (arg == SSG_FLD_TLEN) v = isize;
			else if (arg == SSG_FLD_SEQ_LEN) v = l_seq; else if (arg == SSG_FLD_FLAG) v = flag;
			bool t = v == c;
			if (op == SSG_FOP_NE) t = v != c; else if (op == SSG_FOP_LT) t = v < c; else if (op == SSG_FOP_LE) t = v <= c;
			else if (op == SSG_FOP_GT) t = v > c; else if (op == SSG_FOP_GE) t = v >= c;
			stk = stk << 1 | (t ? 1u : 0u);
		}
	}
	return act && in && (stk & 1u);
}

#ifndef SSG_SEL_DECISION_ONLY   /* (k_depth.h takes sel_keep and leaves the kernel to its own translation unit) */
__global__ void __launch_bounds__(256) ssg_k_bam_select(const uint8_t *chunk, const uint64_t *loc, const uint64_t *key, const ssg_bam_ent_t *ent, int64_t n_rec,
                                                        const ssg_bam_region_t *reg, int32_t n_reg, int32_t n_steps, const ssg_bam_fop_t *prog, int32_t n_prog,
                                                        uint32_t *cnt, const uint64_t *base, uint64_t n_out, uint64_t *out_loc, uint64_t *out_key, ssg_bam_ent_t *out_ent)
{
	__shared__ uint32_t s_kept[4];   /* the kept lanes of the workgroup's four waves */
	const int64_t i = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
	const bool act = i < n_rec;
	uint64_t l = 0; ssg_bam_ent_t e;
	e.tid = e.pos = e.end = 0; e.flag = e.len = e.pad = 0;
	if (act) { l = loc[i]; e = ent[i]; }
	const bool keep = sel_keep(chunk, l & SEL_OFF_MASK, e.end, act, reg, n_reg, n_steps, prog, n_prog);
	const unsigned long long kept = wv_ballot(keep);
	const int wave = (int)(threadIdx.x >> 6);
	if (wv_lane() == 0) s_kept[wave] = (uint32_t)__popcll(kept);
	__syncthreads();
	if (!base) {
		if (threadIdx.x == 0) cnt[blockIdx.x] = s_kept[0] + s_kept[1] + s_kept[2] + s_kept[3];
	} else if (keep) {
		uint64_t w = base[blockIdx.x] + (uint64_t)wv_rank_of(kept);
		if (wave > 0) w += s_kept[0];
		if (wave > 1) w += s_kept[1];
		if (wave > 2) w += s_kept[2];
		if (w < n_out) { out_loc[w] = l; out_key[w] = key[i]; out_ent[w] = e; }
	}
}
#endif
#endif
