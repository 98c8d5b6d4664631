/*
 * k_depth.h -- coverage on the device: the CIGARs of a scanned chunk's records walked into two counters per reference position, regions and windows summed over
 * them, and the lines of `samtools depth' written in HBM (what the kernels stand for in the reference: the pileup loop of samtools
 * 1.3.1 bam2depth.c and bedcov.c, whose output the tests compare).  The chunk lies in the record store, loc[] / key[] / ent[] of its records in device memory as
 * ssg_k_bam_walk and ssg_k_bam_fields (k_bam_scan.h) left them.  Kernels of a translation unit of their own (ssg_depth.cpp): the pinned machine code of the
 * other kernels does not move.
 *
 * The counters of a span [beg, end) of one contig are kept as DIFFERENCES until the span is finished: a run of positions [a, b) is +1 at a - beg and -1 at
 * b - beg (the arrays have end - beg + 1 entries, so the -1 behind the last position has a place), and an exclusive sum over the entries, read one further on,
 * gives the counts.  `span' takes one pair per maximal run of M / = / X / D / N operations, `cov' one pair per maximal run of M / = / X bases that pass the
 * quality test: with min_baseq == 0 that is a run of operations, otherwise the bases are looked at one by one and a lane adds only where passing turns into
 * failing or back.  Integer adds commute: every order of the adds, in LDS or in global memory, gives the same bits.
 *
 *   ssg_k_depth_decide, a lane per record: the filter program (sel_keep of k_bam_select.h without regions), tid >= 0 and n_cigar > 0 make a passing record;
 *     use[i] = 1 when it overlaps the span; the records used, those that matter to a later span (a greater tid, or the same with an end behind the span's), the
 *     records whose key >> 1 (tid, pos) lies below their predecessor's, and -- with min_baseq > 0 -- the smallest offset of a used record whose sequence and
 *     qualities do not lie inside it, go to cnt[0 .. 4); cnt[4] counts the records, passing or not, that begin behind the span (tid < 0, a greater tid, or
 *     pos >= end): in a sorted stream no later chunk adds to the span once there is one (a ballot per wave, one atomic per wave).
 *   ssg_k_depth_accum, a lane per used record (idx[]: their indices, compacted in stream order).  The workgroup's records are neighbours in a coordinate-sorted
 *     file: the least pos and the greatest end of the operations among them, clipped to the span, are found with LDS atomics, and when that stretch has at most `tile' positions the
 *     adds go to two tiles of LDS (tile + 1 dwords each) whose non-zero dwords are then added to global memory by consecutive lanes -- neighbouring workgroups
 *     overlap, so these are atomics too.  A stretch that does not fit (a long N, a sparse region, tile == 0) adds to global memory directly.  Then, with
 *     min_baseq > 0, the wave takes its records one after the other (a wave-uniform loop over the 64 lanes; the record's facts travel by v_readlane): the CIGAR is
 *     read by every lane alike, and the bases of an M / = / X operation that lie inside the span are spread over the lanes.  A base beyond l_seq passes, as
 *     every base of a record with l_seq == 0 does.
 *     Every add is bounds-checked against the span (index <= end - beg) and, in the tile, against the tile.
 *   ssg_k_depth_sums, a wave per segment: the host cuts every (beg, end) pair into segments of at most DEPTH_SEG positions; the lanes read span[] and cov[]
 *     side by side, the wave adds up and lane 0 adds the segment's sums and threshold counts to its pair's row of 64-bit integers.
 *   ssg_k_depth_lens / ssg_k_depth_text, a lane per position: the length of the position's line (0 when it is skipped), and, after an exclusive sum of the
 *     lengths, the line at its offset: name, tab, position + 1, tab, cov, newline.  Every store is bounds-checked against the text's length.
 * Loops whose trip count differs per lane are left by their condition; the loops that hold wave primitives have wave-uniform trip counts.
 */
#ifndef SSG_K_DEPTH_H
#define SSG_K_DEPTH_H
#include "ssg_dev.h"
#define SSG_SEL_DECISION_ONLY
#include "k_bam_select.h"
#include "../../include/ssgpu.h"

#define DEPTH_OFF_MASK (((uint64_t)1 << 40) - 1)
#define DEPTH_SEG 4096          /* positions of a segment of ssg_k_depth_sums */
#define DEPTH_TILE_MAX 8000     /* 2 x 8001 dwords: inside the 64 KB of LDS a workgroup gets without asking */
#define DEPTH_THR_MAX 8

struct depth_seg_t { int64_t beg, end, pair; };   /* positions relative to the span's beg */

SSG_DEVFN uint32_t depth_ld32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
SSG_DEVFN bool depth_ref_op(uint32_t op) { return op == 0u || op == 2u || op == 3u || op == 7u || op == 8u; }   /* M D N = X */
SSG_DEVFN bool depth_base_op(uint32_t op) { return op == 0u || op == 7u || op == 8u; }                         /* M = X */
SSG_DEVFN bool depth_query_op(uint32_t op) { return op == 0u || op == 1u || op == 4u || op == 7u || op == 8u; } /* M I S = X */

__global__ void __launch_bounds__(256) ssg_k_depth_decide(const uint8_t *chunk, const uint64_t *loc, const uint64_t *key, const ssg_bam_ent_t *ent, int64_t n_rec,
                                                          const ssg_bam_fop_t *prog, int32_t n_prog, int32_t s_tid, int32_t s_beg, int32_t s_end, int32_t min_baseq,
                                                          uint8_t *use, uint32_t *idx, unsigned long long *cnt)
{
	const int64_t i = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
	const bool act = i < n_rec;
	uint64_t l = 0, k0 = 0, k1 = 0; ssg_bam_ent_t e;
	e.tid = e.pos = e.end = 0; e.flag = e.len = e.pad = 0;
	if (act) { l = loc[i]; e = ent[i]; k1 = key[i] >> 1; k0 = i > 0 ? key[i - 1] >> 1 : k1; }
	const uint64_t off = l & DEPTH_OFF_MASK;
	bool pass = sel_keep(chunk, off, e.end, act, (const ssg_bam_region_t*)0, 0, 0, prog, n_prog);
	uint32_t x[6] = { 0, 0, 0, 0, 0, 0 };
	if (act) memcpy(x, chunk + off, 24);   /* block_size, tid, pos, bin_mq_nl, flag_nc, l_seq */
	const uint32_t bs = x[0], lq = x[3] & 0xffu, nc = x[4] & 0xffffu, ls = x[5];
	pass = pass && e.tid >= 0 && nc > 0;
	const bool used = pass && e.tid == s_tid && e.pos < s_end && e.end > s_beg;
	const bool later = pass && (e.tid > s_tid || (e.tid == s_tid && e.end > s_end));
	const bool desc = act && k1 < k0;
	const bool bad = used && min_baseq > 0 && 32u + (uint64_t)lq + 4u * (uint64_t)nc + ((uint64_t)ls + 1u) / 2u + (uint64_t)ls > (uint64_t)bs;
	if (act) { use[i] = used ? 1 : 0; idx[i] = (uint32_t)i; }
	const bool behind = act && (e.tid < 0 || e.tid > s_tid || (e.tid == s_tid && e.pos >= s_end));
	const unsigned long long bu = wv_ballot(used), bl = wv_ballot(later), bd = wv_ballot(desc), bb = wv_ballot(behind);
	if (wv_lane() == 0) {
		if (bu) atomicAdd(cnt + 0, (unsigned long long)__popcll(bu));
		if (bl) atomicAdd(cnt + 1, (unsigned long long)__popcll(bl));
		if (bd) atomicAdd(cnt + 2, (unsigned long long)__popcll(bd));
		if (bb) atomicAdd(cnt + 4, (unsigned long long)__popcll(bb));
	}
	if (bad) atomicMin(cnt + 3, (unsigned long long)off);
}

/* +1 at a and -1 at b for the run [a, b) of reference positions, clipped to the span [s_beg, s_end); in the tile when there is one (t_lo: the position of its
 * first dword, t_n: its dwords) */
SSG_DEVFN void depth_add_run(int64_t a, int64_t b, int32_t s_beg, int32_t s_end, uint32_t *g, uint32_t *t, int64_t t_lo, int32_t t_n)
{
	if (a < s_beg) a = s_beg;
	if (b > s_end) b = s_end;
	if (a >= b) return;
	const int64_t n = (int64_t)s_end - (int64_t)s_beg;
	if (t) {
		const int64_t ia = a - t_lo, ib = b - t_lo;
		if (ia >= 0 && ib < t_n) { atomicAdd(t + ia, 1u); atomicAdd(t + ib, 0xffffffffu); }
	} else {
		const int64_t ia = a - s_beg, ib = b - s_beg;
		if (ia >= 0 && ib <= n) { atomicAdd(g + ia, 1u); atomicAdd(g + ib, 0xffffffffu); }
	}
}
SSG_DEVFN void depth_add_one(int64_t p, uint32_t v, int32_t s_beg, int32_t s_end, uint32_t *g, uint32_t *t, int64_t t_lo, int32_t t_n)
{
	if (t) { const int64_t ip = p - t_lo; if (ip >= 0 && ip < t_n) atomicAdd(t + ip, v); }
	else { const int64_t ip = p - s_beg; if (ip >= 0 && ip <= (int64_t)s_end - (int64_t)s_beg) atomicAdd(g + ip, v); }
}

__global__ void __launch_bounds__(256) ssg_k_depth_accum(const uint8_t *chunk, const uint64_t *loc, const ssg_bam_ent_t *ent, const uint32_t *idx, uint32_t n_used,
                                                         int32_t s_beg, int32_t s_end, int32_t min_baseq, int32_t tile, uint32_t *d_span, uint32_t *d_cov)
{
#ifdef SSG_EMU
	uint32_t *lds = (uint32_t*)emu::dyn_lds;
#else
	extern __shared__ uint32_t ssg_depth_lds[];
	uint32_t *lds = ssg_depth_lds;
#endif
	__shared__ int32_t s_lohi[2];
	const uint32_t j = blockIdx.x * 256u + threadIdx.x;
	const bool act = j < n_used;
	uint64_t off = 0; int32_t pos = 0; uint32_t lq = 0, nc = 0, ls = 0;
	if (act) {
		const uint32_t i = idx[j];
		off = loc[i] & DEPTH_OFF_MASK; pos = ent[i].pos;
		uint32_t x[6]; memcpy(x, chunk + off, 24);
		lq = x[3] & 0xffu; nc = x[4] & 0xffffu; ls = x[5];
	}
	/* where the record's operations end (ent[].end is bam_endpos: pos + 1 for a record flagged unmapped, whatever its CIGAR says) */
	int64_t rend = pos;
	for (uint32_t k = 0; k < nc; ++k) { const uint32_t c = depth_ld32(chunk + off + 36 + lq + 4 * (uint64_t)k); if (depth_ref_op(c & 0xfu)) rend += (int64_t)(c >> 4); }
	/* the stretch of the workgroup's records inside the span */
	if (threadIdx.x == 0) { s_lohi[0] = s_end; s_lohi[1] = s_beg; }
	__syncthreads();
	if (act && tile > 0) { atomicMin(&s_lohi[0], pos > s_beg ? pos : s_beg); atomicMax(&s_lohi[1], rend < s_end ? (int32_t)rend : s_end); }
	__syncthreads();
	const int64_t t_lo = s_lohi[0]; const int64_t stretch = (int64_t)s_lohi[1] - t_lo;
	const bool tiled = tile > 0 && stretch >= 0 && stretch <= (int64_t)tile;
	const int32_t t_n = tiled ? (int32_t)stretch + 1 : 0;
	uint32_t *const ts = tiled ? lds : (uint32_t*)0, *const tc = tiled ? lds + (tile + 1) : (uint32_t*)0;
	if (tiled) {
		for (int32_t k = (int32_t)threadIdx.x; k < t_n; k += 256) { ts[k] = 0; tc[k] = 0; }
		__syncthreads();
	}
	/* a lane per record: the runs of reference-consuming operations, and (without a quality test) of base-to-base operations */
	{
		const uint8_t *cig = chunk + off + 36 + lq;
		/* (S, I, H and P consume no reference: they end no run.  The reference-consuming operations of a record follow one another without a gap, so span has one run
		 * a record; a D or an N ends a run of cov) */
		int64_t r = pos, ca = -1;   /* ca: where the open run of cov began */
		const bool runs = min_baseq == 0;
		for (uint32_t k = 0; k < nc; ++k) {
			const uint32_t c = depth_ld32(cig + 4 * (uint64_t)k), op = c & 0xfu; const int64_t len = (int64_t)(c >> 4);
			const bool ro = depth_ref_op(op), bo = depth_base_op(op);
			if (runs && ro && !bo && ca >= 0) { depth_add_run(ca, r, s_beg, s_end, d_cov, tc, t_lo, t_n); ca = -1; }
			if (runs && bo && ca < 0) ca = r;
			if (ro) r += len;
		}
		if (act) depth_add_run(pos, rend, s_beg, s_end, d_span, ts, t_lo, t_n);
		if (ca >= 0) depth_add_run(ca, r, s_beg, s_end, d_cov, tc, t_lo, t_n);
	}
	/* with a quality test: a wave per record, its bases over the lanes */
	if (min_baseq > 0) {
		const int lane = wv_lane();
		for (int w = 0; w < 64; ++w) {   /* (a lane without a record has n_cigar == 0: nothing is read for it) */
			const uint64_t w_off = (uint64_t)wv_get64((long long)off, w);
			const int64_t w_pos = wv_get(pos, w);
			const uint32_t w_lq = (uint32_t)wv_get((int)lq, w), w_nc = (uint32_t)wv_get((int)nc, w), w_ls = (uint32_t)wv_get((int)ls, w);
			const uint8_t *cig = chunk + w_off + 36 + w_lq, *qual = cig + 4 * (uint64_t)w_nc + ((uint64_t)w_ls + 1u) / 2u;
			int64_t r = w_pos, q = 0;
			for (uint32_t k = 0; k < w_nc; ++k) {
				const uint32_t c = depth_ld32(cig + 4 * (uint64_t)k), op = c & 0xfu; const int64_t len = (int64_t)(c >> 4);
				if (depth_base_op(op)) {
					/* bases t0 .. t1 of the operation lie inside the span; base t passes when it has no quality byte or the byte is at least min_baseq */
					const int64_t t0 = r < s_beg ? (int64_t)s_beg - r : 0, t1 = r + len > s_end ? (int64_t)s_end - r : len;
					for (int64_t t = t0 + lane; t <= t1; t += 64) {
						const bool cur = t < t1 && (q + t >= (int64_t)w_ls || (int32_t)qual[q + t] >= min_baseq);
						const bool prev = t > t0 && (q + t - 1 >= (int64_t)w_ls || (int32_t)qual[q + t - 1] >= min_baseq);
						if (cur != prev) depth_add_one(r + t, cur ? 1u : 0xffffffffu, s_beg, s_end, d_cov, tc, t_lo, t_n);
					}
				}
				if (depth_ref_op(op)) r += len;
				if (depth_query_op(op)) q += len;
			}
		}
	}
	if (tiled) {
		__syncthreads();
		const int64_t g0 = t_lo - (int64_t)s_beg, n = (int64_t)s_end - (int64_t)s_beg;
		for (int32_t k = (int32_t)threadIdx.x; k < t_n; k += 256) {
			const uint32_t vs = ts[k], vc = tc[k];
			if (g0 + k >= 0 && g0 + k <= n) { if (vs) atomicAdd(d_span + g0 + k, vs); if (vc) atomicAdd(d_cov + g0 + k, vc); }
		}
	}
}

SSG_DEVFN unsigned long long depth_wave_sum64(unsigned long long v)
{
	for (int d = 1; d < 64; d <<= 1) v += (unsigned long long)wv_shfl64_xor((long long)v, d);
	return v;
}

/* four waves a workgroup, a segment each; out: 2 + n_thr values a pair */
__global__ void __launch_bounds__(256) ssg_k_depth_sums(const uint32_t *span, const uint32_t *cov, int64_t n_pos, const depth_seg_t *seg, int64_t n_seg,
                                                        const uint32_t *thr, int32_t n_thr, unsigned long long *out, int64_t n_pair)
{
	const int64_t s = (int64_t)blockIdx.x * 4 + (int64_t)(threadIdx.x >> 6);
	const bool act = s < n_seg;   /* (wave-uniform) */
	int64_t b = 0, e = 0, pair = 0;
	if (act) { b = seg[s].beg; e = seg[s].end; pair = seg[s].pair; }
	if (b < 0) b = 0;
	if (e > n_pos) e = n_pos;
	uint32_t th[DEPTH_THR_MAX]; int cn[DEPTH_THR_MAX];
	SSG_UNROLL for (int k = 0; k < DEPTH_THR_MAX; ++k) { th[k] = k < n_thr ? thr[k] : 0u; cn[k] = 0; }
	unsigned long long ss = 0, sc = 0;
	for (int64_t p = b + wv_lane(); p < e; p += 64) {
		const uint32_t vs = span[p], vc = cov[p];
		ss += vs; sc += vc;
		SSG_UNROLL for (int k = 0; k < DEPTH_THR_MAX; ++k) cn[k] += vc >= th[k] ? 1 : 0;
	}
	ss = depth_wave_sum64(ss); sc = depth_wave_sum64(sc);
	SSG_UNROLL for (int k = 0; k < DEPTH_THR_MAX; ++k) cn[k] = wv_sum(cn[k]);
	if (act && wv_lane() == 0 && pair >= 0 && pair < n_pair) {
		unsigned long long *o = out + pair * (2 + (int64_t)n_thr);
		if (ss) atomicAdd(o + 0, ss);
		if (sc) atomicAdd(o + 1, sc);
		SSG_UNROLL for (int k = 0; k < DEPTH_THR_MAX; ++k) if (k < n_thr && cn[k]) atomicAdd(o + 2 + k, (unsigned long long)cn[k]);
	}
}

SSG_DEVFN uint32_t depth_digits(uint32_t v) { uint32_t d = 1; while (v >= 10u) { v /= 10u; ++d; } return d; }

/* positions i0 .. i0 + n of the span (relative to its beg; position0: the reference position of entry 0) */
__global__ void __launch_bounds__(256) ssg_k_depth_lens(const uint32_t *span, const uint32_t *cov, int64_t i0, int64_t n, int64_t position0, uint32_t name_len, int32_t all, uint32_t *len)
{
	const int64_t t = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
	if (t >= n) return;
	const int64_t i = i0 + t;
	len[t] = all || span[i] > 0 ? name_len + depth_digits((uint32_t)(position0 + i + 1)) + depth_digits(cov[i]) + 3u : 0u;
}
__global__ void __launch_bounds__(256) ssg_k_depth_text(const uint32_t *cov, int64_t i0, int64_t n, int64_t position0, const uint8_t *name, uint32_t name_len,
                                                        const uint32_t *len, const uint64_t *off, uint8_t *out, uint64_t out_len)
{
	const int64_t t = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
	if (t >= n) return;
	const uint32_t ln = len[t];
	const uint64_t o = off[t];
	if (ln == 0 || o + ln > out_len) return;
	const int64_t i = i0 + t;
	uint8_t *w = out + o;
	for (uint32_t k = 0; k < name_len; ++k) w[k] = name[k];
	w += name_len; *w++ = '\t';
	uint32_t v = (uint32_t)(position0 + i + 1), d = depth_digits(v);
	for (uint32_t k = d; k > 0; --k) { w[k - 1] = (uint8_t)('0' + v % 10u); v /= 10u; }
	w += d; *w++ = '\t';
	v = cov[i]; d = depth_digits(v);
	for (uint32_t k = d; k > 0; --k) { w[k - 1] = (uint8_t)('0' + v % 10u); v /= 10u; }
	w += d; *w = '\n';
}
#endif
