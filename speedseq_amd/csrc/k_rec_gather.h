/*
 * k_rec_gather.h -- the payload of `sambamba sort`'s output blocks built in HBM (what the kernel stands for in the
 * reference: bgzf_write's copy of a record into the block buffer, htslib bgzf.c): the records of the input lie in the chunks they arrived in
 * (ssg_recs_append), record i of the sorted order at loc[i] = chunk << 40 | offset of its block_size word, and occupies bytes cum[i] .. cum[i+1]
 * of the sorted stream.  ssg_k_rec_gather writes stream bytes v0 .. v1 to out[0 .. v1 - v0).
 * A kernel of a translation unit of its own (ssg_rec_gather.cpp): the pinned machine code of the deflate, CRC-32 and framing kernels does not move.
 *
 * A copy with a sorted destination and scattered sources, so it is organised by destination:
 *   - a workgroup takes RG_TILE bytes of the output, in RG_ITERS passes of 256 aligned 16-byte granules (4 KB: the wave's stores are 1 KB each,
 *     lane l next to lane l + 1);
 *   - the first and the last record of a pass are found by bisection in cum[], the same for every lane (the second search starts at the first's
 *     answer; the next pass starts where this one ended);
 *   - a lane finds the record its granule starts in by a bisection inside that range -- about a dozen records of 350 bytes, four steps, the
 *     same count for every lane: the trip count comes from the range, not from the lane -- and then walks: 16 bytes from where it is in the record
 *     (an unaligned load; the 16 bytes of slack behind every chunk make it safe wherever in a record it starts), shifted to the granule's first
 *     free byte and merged in registers, on to the next record until the granule is full.  One record for most granules of BAM records, up to 16
 *     for records of one byte.  The walk is left by a flag and one test per wave;
 *   - a full granule is one 16-byte store; the stream's last, partial granule is written byte by byte.  Nothing is stored outside out[0 .. v1 - v0).
 * The host has checked every loc / cum against the chunks (ssg_recs_order), so no load leaves an allocation.
 * A streaming kernel -- every byte read once through L2, written once -- expected, not yet measured, to be small beside ssg_k_bgzf_deflate on
 * the same payload.
 */
#ifndef SSG_K_REC_GATHER_H
#define SSG_K_REC_GATHER_H
#include "ssg_dev.h"

#define RG_ITERS 4
#define RG_TILE (RG_ITERS * 256 * 16)   /* output bytes per workgroup */
#define RG_OFF_MASK (((uint64_t)1 << 40) - 1)

typedef unsigned __int128 rg_u128;
struct rg_pair64_t { uint64_t lo, hi; };
SSG_DEVFN rg_u128 rg_load16(const uint8_t *p) { rg_pair64_t w; memcpy(&w, p, 16); return (rg_u128)w.lo | (rg_u128)w.hi << 64; }

/* the largest i in [a, b] with cum[i] <= s (cum[a] <= s): the record that holds stream byte s, whatever records without bytes lie before it */
SSG_DEVFN int64_t rg_find(const uint64_t *cum, int64_t a, int64_t b, uint64_t s)
{
	while (a < b) { const int64_t m = (a + b + 1) >> 1; if (cum[m] <= s) a = m; else b = m - 1; }
	return a;
}

__global__ void __launch_bounds__(256) ssg_k_rec_gather(const uint8_t *const *chunk, const uint64_t *loc, const uint64_t *cum, int64_t n, uint64_t v0, uint64_t v1, uint8_t *out)
{
	const uint64_t N = v1 - v0;
	uint64_t t0 = (uint64_t)blockIdx.x * RG_TILE;   /* first output byte of the pass */
	if (t0 >= N || n <= 0) return;
	int64_t lo = rg_find(cum, 0, n - 1, v0 + t0);
	for (int it = 0; it < RG_ITERS && t0 < N; ++it, t0 += 256 * 16) {
		const uint64_t t1 = t0 + 256 * 16 < N ? t0 + 256 * 16 : N;
		const int64_t hi = rg_find(cum, lo, n - 1, v0 + t1 - 1);
		int steps = 0; while (((int64_t)1 << steps) < hi - lo + 1) ++steps;
		const uint64_t d = t0 + 16 * (uint64_t)threadIdx.x;   /* this lane's granule: out[d .. d + 16) */
		const uint64_t s = v0 + d;
		bool act = d < N;
		/* (a lane behind the end searches for the last byte: every address stays inside cum[lo .. hi]) */
		const uint64_t sf = act ? s : v0 + t1 - 1;
		int64_t a = lo, b = hi;
		for (int k = 0; k < steps; ++k) { const int64_t m = (a + b + 1) >> 1; const bool le = cum[m] <= sf; a = le ? m : a; b = le ? b : m - 1; }
		int64_t i = a; uint32_t filled = 0; rg_u128 acc = 0;
		while (wv_ballot(act)) {
			if (act) {
				const uint64_t c0 = cum[i], c1 = cum[i + 1], at = s + filled, l = loc[i];
				const uint64_t avail = c1 - at;
				const uint32_t take = avail < 16 - filled ? (uint32_t)avail : 16 - filled;
				const rg_u128 w = rg_load16(chunk[l >> 40] + (l & RG_OFF_MASK) + (at - c0));
				acc = (acc & ((((rg_u128)1) << (8 * filled)) - 1)) | (w << (8 * filled));   /* (what lies behind the record's bytes in w is replaced by the next piece) */
				filled += take; ++i;
				act = filled < 16 && i < n;
			}
		}
		if (d + 16 <= N) { ssg_q16_t q; q.v[0] = (uint32_t)acc; q.v[1] = (uint32_t)(acc >> 32); q.v[2] = (uint32_t)(acc >> 64); q.v[3] = (uint32_t)(acc >> 96); *(ssg_q16_t*)(out + d) = q; }
		else if (d < N) { for (uint32_t k = 0; k < (uint32_t)(N - d); ++k) out[d + k] = (uint8_t)(acc >> (8 * k)); }
		lo = hi;
	}
}
#endif
