/*
 * k_bam_scan.h -- the records of a chunk of inflated BAM found on the device (what the kernels stand for in the reference: bam_read1's
 * walk from block_size to block_size, htslib sam.c, and the fields hts_idx_push and bam1_lt read of a record).  The chunk lies in the record store
 * (ssg_recs_append_bgzf: BGZF members inflated into it, never copied to the host); the stream of records is chunk[first .. total).
 * Kernels of a translation unit of their own (ssg_bam_scan.cpp): the pinned machine code of the other kernels does not move.
 *
 * Where a record begins is known only from the record before it, so one walk of the whole stream would be one lane's work.  Every mainstream writer starts a
 * BGZF block at a record (bgzf_flush_try), so the members' offsets hint[] are places where a record is expected to begin, and the intervals between them are
 * walked side by side:
 *   - ssg_k_bam_walk, a lane per interval [hint[b], hint[b+1]): it enters at hint[b] (at `first' where that lies behind: the header's bytes come before the
 *     first record), goes from block_size word to block_size word and leaves when it reaches hint[b+1].  It runs twice: first it counts (loc == NULL) and
 *     leaves the count, the offset it stopped at and a state per interval; after an exclusive scan of the counts it writes loc[] = tag | offset.
 *     The states: BS_OK; BS_SMALL (a block_size below 32); BS_PAST (a record, or its block_size word, runs past `total'); BS_SKEW (the walk passed hint[b+1]
 *     without landing on it: no record begins there -- a property of the file; the host reports the first interval that is not BS_OK, and up to there every
 *     walk entered at a true record).
 *     Every load is bounds-checked against `total' before it is issued: a lane that entered in the middle of a record reads garbage sizes and stops at the
 *     first one that does not fit.  An interval without bytes (the end-of-file marker inside a concatenated file) yields nothing.  The trip count differs per
 *     lane: the loop is left by a flag and one test per wave.
 *   - ssg_k_bam_fields, a lane per record: the 36 fixed bytes and the CIGAR; key = bam_sort_key, end = bam_endpos (host/bamio.h), bit for bit.  A record
 *     whose l_qname + 4 n_cigar does not fit its block_size reads no CIGAR and leaves the smallest such offset in *bad.
 * About 180 dependent loads per lane for members of 64 KB of 2x150 records: latency-bound and small beside the inflate of the same members (an estimate,
 * DESIGN.md section 6.2).
 */
#ifndef SSG_K_BAM_SCAN_H
#define SSG_K_BAM_SCAN_H
#include "ssg_dev.h"
#include "../../include/ssgpu.h"

#define BS_OFF_MASK (((uint64_t)1 << 40) - 1)
#define BS_OK 0u
#define BS_SMALL 1u
#define BS_PAST 2u
#define BS_SKEW 3u

__global__ void __launch_bounds__(256) ssg_k_bam_walk(const uint8_t *chunk, uint64_t total, const uint64_t *hint, int64_t n_hints, uint64_t first, uint64_t *cnt, uint64_t *stop, uint32_t *state,
                                                      const uint64_t *base, uint64_t tag, uint64_t n_loc, uint64_t *loc)
{
	const int64_t b = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
	bool act = b < n_hints;
	uint64_t off = 0, end = 0, w = 0, n = 0; uint32_t st = BS_OK; bool walked = false;
	if (act) {
		const uint64_t h0 = hint[b];
		end = hint[b + 1]; off = h0 > first ? h0 : first;
		act = off < end; walked = act;
		if (loc) w = base[b];
	}
	while (wv_ballot(act)) {
		if (act) {
			const bool word = off + 4 <= total;
			uint32_t bs = 0;
			if (word) memcpy(&bs, chunk + off, 4);
			const bool fits = word && bs >= 32u && (uint64_t)bs <= total - off - 4;
			if (fits) {
				if (loc && w < n_loc) loc[w] = tag | off;
				++w; ++n; off += 4 + (uint64_t)bs;
			} else st = word && bs < 32u ? BS_SMALL : BS_PAST;
			act = fits && off < end;
		}
	}
	if (b < n_hints && !loc) {
		if (st == BS_OK && walked && off != end) st = BS_SKEW;
		cnt[b] = n; stop[b] = walked ? off : end; state[b] = st;
	}
}

__global__ void __launch_bounds__(256) ssg_k_bam_fields(const uint8_t *chunk, const uint64_t *loc, int64_t n_rec, uint64_t *key, ssg_bam_ent_t *ent, unsigned long long *bad)
{
	const int64_t i = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
	bool act = i < n_rec;
	const uint8_t *cig = chunk; uint32_t nc = 0, k = 0; int32_t rl = 0, pos = 0; ssg_bam_ent_t e;
	e.tid = e.pos = e.end = 0; e.flag = e.len = e.pad = 0;
	if (act) {
		const uint64_t off = loc[i] & BS_OFF_MASK;
		uint32_t x[5]; memcpy(x, chunk + off, 20);   /* block_size, tid, pos, bin_mq_nl, flag_nc: the walk has seen that 4 + block_size >= 36 bytes lie inside */
		const uint32_t bs = x[0], l_qname = x[3] & 0xffu, flag = x[4] >> 16;
		nc = x[4] & 0xffffu; pos = (int32_t)x[2];
		e.tid = (int32_t)x[1]; e.pos = pos; e.flag = flag; e.len = 4u + bs;
		key[i] = (uint64_t)(int64_t)e.tid << 32 | (uint64_t)(uint32_t)((x[2] + 1u) << 1) | (flag & 0x10u ? 1u : 0u);
		if (l_qname + 4u * nc > bs - 32u) { atomicMin(bad, (unsigned long long)off); nc = 0; }
		if ((flag & 4u) || nc == 0) { nc = 0; rl = 1; }
		cig = chunk + off + 36 + l_qname;
		act = nc > 0;
	}
	while (wv_ballot(act)) {
		if (act) {
			uint32_t v; memcpy(&v, cig + 4 * (uint64_t)k, 4);
			const uint32_t op = v & 0xfu;
			if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += (int32_t)(v >> 4);
			++k; act = k < nc;
		}
	}
	if (i < n_rec) { e.end = pos + rl; ent[i] = e; }
}
#endif
