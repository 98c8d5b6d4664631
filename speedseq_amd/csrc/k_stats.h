/*
 * k_stats.h -- the QC tables of `samtools stats' counted on the device (what the kernels stand for in the reference: collect_stats, collect_orig_read_stats,
 * count_indels, update_checksum and round_buffer_* of samtools 1.3.1 stats.c, whose output the tests compare).  The chunk lies in the record store, loc[] of its
 * records in device memory as ssg_k_bam_walk (k_bam_scan.h) left it.  Kernels of a translation unit of their own (ssg_stats.cpp): the pinned machine code of the
 * other kernels does not move.  Everything but the coverage histogram is a sum of integers: every order of the adds, in LDS or in global memory, gives the same bits.
 *
 *   ssg_k_stats_decide, a lane per record: the filter program (sel_keep of k_bam_select.h without regions), collect_stats' gate (secondary, l_seq == 0, duplicate),
 *     the unclipped length, the classes of collect_orig_read_stats, one walk of the CIGAR (hard clips, M + I, count_indels) and one of the aux area (the first NM,
 *     k_b2f.h's type table).  The C and G bases of a record are counted here, 16 packed bases a step.  Scalar counts go through ballots, scalar sums through wave
 *     reductions, one atomic per wave each; the rare events (rl, id, ic, isize, and the GC range as + 1 and - 1 into a difference array of 200 entries) go straight
 *     to global 64-bit atomics, every index checked against its table.  What the later kernels need of a record is left in cls[] (bit 0: it passed the filter
 *     and fits its block_size), pb[] (where its sequence begins, l_seq, fragment and strand; l_seq == 0 for a record that adds no bases) and use[] (it is covered).
 *     The four refusals are atomicMins of the record's offset into err[0 .. 4); err[4] becomes the longest l_seq with bases to add.  The host puts the small tables
 *     back when there is a refusal, so nothing here has to be undone.
 *   ssg_k_stats_bases, the hot one: a workgroup owns a tile of `tile' cycles (at most 32) and a slab of `slab' records, and keeps quals[2][tile][256] and
 *     bases[tile][6] of them as 32-bit counters in LDS.  A half-wave takes a record at a time and a lane is a cycle: the 32 lanes of a half-wave hit 32 different rows,
 *     and they read consecutive bytes of the record, ascending or -- a reverse read -- descending.  A quality row is 257 dwords and a base row 7, so that one quality
 *     value (or one base) across the cycles lies on 32 different banks.  A counter takes at most one add a record: a slab cannot overflow it.  The non-zero dwords are
 *     then added to global memory as 64-bit integers by consecutive lanes (rows checked against the tables).  The tile is 2 x 32 x 257 + 32 x 7 dwords = 66 688 bytes:
 *     two workgroups a CU (160 KB).  Results depend on neither tile nor slab (SSG_STATS_TILE, SSG_STATS_SLAB).
 *   ssg_k_stats_crc, a lane per record that passed: the three CRC-32s of update_checksum with the slice-by-4 tables of k_bgzf_frame.h in LDS, summed over the wave.
 *   ssg_k_stats_ckeys, a lane per covered record (kept[]: their indices, compacted in stream order): its key (tid, pos) and whether it lies below its predecessor's.
 *   ssg_k_stats_cov_add: + 1 at pos and - 1 at pos + l_seq of the window's difference array; ssg_k_stats_cov_hist: the non-zero depths (the exclusive sum of the
 *     differences, read one entry further on) into LDS bins through coverage_idx, one flush per workgroup; ssg_k_stats_cov_carry: the window moved on by `span'
 *     positions -- the depth at the new first position and the differences of the slack behind it.
 * Loops whose trip count differs per lane are left by their condition or by a flag and hold no wave primitive.
 */
#ifndef SSG_K_STATS_H
#define SSG_K_STATS_H
#include "ssg_dev.h"
#define SSG_SEL_DECISION_ONLY
#include "k_bam_select.h"
#define SSG_BZF_TABLES_ONLY
#include "k_bgzf_frame.h"
#include "../../include/ssgpu.h"

#define STATS_OFF_MASK (((uint64_t)1 << 40) - 1)
#define STATS_TILE_MAX 32
#define STATS_QROW 257
#define STATS_BROW 7
#define STATS_COV_MAX 8192      /* bins of the coverage histogram: 32 KB of LDS */
enum { STATS_ERR_FIT, STATS_ERR_LONG, STATS_ERR_NOCIGAR, STATS_ERR_CYCLE, STATS_PUSH_MAX, STATS_ERR_N = 8 };

struct stats_tab_t { unsigned long long *sc, *gc, *isz, *rl, *id, *ic, *quals, *bases, *cov; int32_t rows, n_isize; };   /* rows: max_len + 1 */
struct stats_pb_t { uint64_t seq; uint32_t ls, fl; };   /* seq: the offset of the packed sequence in the chunk; fl: 1 last fragment, 2 reverse */

SSG_DEVFN uint32_t stats_ld32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
SSG_DEVFN unsigned long long stats_wave_sum64(unsigned long long v)
{
	for (int d = 1; d < 64; d <<= 1) v += (unsigned long long)wv_shfl64_xor((long long)v, d);
	return v;
}
SSG_DEVFN uint32_t stats_wave_sum32(uint32_t v)   /* modulo 2^32: the checksums wrap */
{
	for (int d = 1; d < 64; d <<= 1) v += (uint32_t)wv_shfl((int)v, wv_lane() ^ d);
	return v;
}
/* (every lane of the wave calls these) */
SSG_DEVFN void stats_count(unsigned long long *sc, int slot, bool p)
{
	const unsigned long long b = wv_ballot(p);
	if (wv_lane() == 0 && b) atomicAdd(sc + slot, (unsigned long long)__popcll(b));
}
SSG_DEVFN void stats_sum(unsigned long long *sc, int slot, unsigned long long v)
{
	v = stats_wave_sum64(v);
	if (wv_lane() == 0 && v) atomicAdd(sc + slot, v);
}
/* the 4-bit codes 2 (C) and 4 (G) among the first n of a sequence's packed bases */
SSG_DEVFN uint32_t stats_gc_count(const uint8_t *seq, uint32_t n)
{
	const uint64_t ones = 0x1111111111111111ull;
	const uint32_t nb = n >> 1;
	uint32_t g = 0, k = 0;
	for (; k + 8 <= nb; k += 8) {
		uint64_t w; memcpy(&w, seq + k, 8);
		const uint64_t c = w ^ (2 * ones), d = w ^ (4 * ones);
		g += 32u - (uint32_t)__popcll((c | c >> 1 | c >> 2 | c >> 3) & ones) - (uint32_t)__popcll((d | d >> 1 | d >> 2 | d >> 3) & ones);
	}
	for (; k < nb; ++k) { const uint32_t b = seq[k]; g += ((b >> 4) == 2u || (b >> 4) == 4u ? 1u : 0u) + ((b & 15u) == 2u || (b & 15u) == 4u ? 1u : 0u); }
	if (n & 1u) { const uint32_t b = seq[nb] >> 4; g += b == 2u || b == 4u ? 1u : 0u; }
	return g;
}

__global__ void __launch_bounds__(256) ssg_k_stats_decide(const uint8_t *chunk, const uint64_t *loc, int64_t n_rec, const ssg_bam_fop_t *prog, int32_t n_prog, stats_tab_t T,
                                                          uint8_t *cls, stats_pb_t *pb, uint8_t *use, uint32_t *idx, unsigned long long *err)
{
	const int64_t i = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
	const bool act = i < n_rec;
	const uint64_t off = act ? loc[i] & STATS_OFF_MASK : 0;
	const bool pass = sel_keep(chunk, off, 0, act, (const ssg_bam_region_t*)0, 0, 0, prog, n_prog);
	uint32_t x[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
	if (act) memcpy(x, chunk + off, 36);   /* block_size, tid, pos, bin_mq_nl, flag_nc, l_seq, mtid, mpos, isize */
	const uint32_t bs = x[0], lq = x[3] & 0xffu, mapq = x[3] >> 8 & 0xffu, nc = x[4] & 0xffffu, flag = x[4] >> 16, ls = x[5];
	const int64_t L = (int64_t)T.rows - 1;
	const uint64_t aux0 = 32u + (uint64_t)lq + 4u * (uint64_t)nc + ((uint64_t)ls + 1u) / 2u + (uint64_t)ls;   /* where the aux area begins, from the record's body */
	const bool fit = act && aux0 <= (uint64_t)bs;
	if (act && !fit) atomicMin(err + STATS_ERR_FIT, (unsigned long long)off);
	const uint8_t *const body = chunk + off + 4, *const cig = body + 32 + lq, *const seq = cig + 4 * (uint64_t)nc;
	const bool kept = pass && fit;
	const bool far = kept && !(flag & 0x100u) && ls > 0;   /* the record gets as far as the unclipped length */
	const bool orig = far && !(flag & 0x900u), mapped = far && !(flag & 4u);
	const bool fwd = !(flag & 0x10u);
	const int f1 = (flag & 0x40u) ? 0 : 1;   /* count_indels: IS_READ1 or not */
	/* one walk of the CIGAR */
	int64_t hard = 0, mi = 0, cyc = 0; bool bad_cycle = false;
	if (far) for (uint32_t k = 0; k < nc; ++k) {
		const uint32_t c = stats_ld32(cig + 4 * (uint64_t)k), op = c & 0xfu; const int64_t len = (int64_t)(c >> 4);
		if (op == 5u) hard += len;
		if (mapped && (op == 0u || op == 1u)) mi += len;
		if (mapped && len > 0) {
			if (op == 1u) {
				const int64_t ix = fwd ? cyc : (int64_t)ls - cyc - len;
				if (ix < 0 || ix > L) bad_cycle = true;
				else { atomicAdd(T.ic + (int64_t)f1 * T.rows + ix, 1ull); if (len <= SSG_STATS_NINDEL) atomicAdd(T.id + (len - 1), 1ull); }
				cyc += len;
			} else if (op == 2u) {
				const int64_t ix = fwd ? cyc - 1 : (int64_t)ls - cyc - 1;
				if (ix > L) bad_cycle = true;
				else if (ix >= 0) { atomicAdd(T.ic + (int64_t)(2 + f1) * T.rows + ix, 1ull); if (len <= SSG_STATS_NINDEL) atomicAdd(T.id + SSG_STATS_NINDEL + (len - 1), 1ull); }
			} else if (op != 3u && op != 5u && op != 6u) cyc += len;
		}
	}
	const int64_t unclipped = (int64_t)ls + hard;
	const bool too_long = far && unclipped > L;
	if (too_long) atomicMin(err + STATS_ERR_LONG, (unsigned long long)off);
	if (mapped && nc == 0) atomicMin(err + STATS_ERR_NOCIGAR, (unsigned long long)off);
	if (bad_cycle) atomicMin(err + STATS_ERR_CYCLE, (unsigned long long)off);
	const bool ok = far && !too_long;   /* (l_seq <= max_len from here on) */
	/* collect_orig_read_stats */
	const bool count = orig && ok;
	const bool last = (flag & 0x80u) != 0;
	if (count) {
		atomicAdd(T.rl + unclipped, 1ull);
		const uint32_t g = stats_gc_count(seq, ls);
		const int32_t lo = (int32_t)((uint64_t)g * (SSG_STATS_NGC - 1) / ls); int32_t hi = (int32_t)(((uint64_t)g + 1) * (SSG_STATS_NGC - 1) / ls);
		if (hi > SSG_STATS_NGC - 1) hi = SSG_STATS_NGC - 1;
		if (lo < hi) { unsigned long long *gc = T.gc + (last ? SSG_STATS_NGC : 0); atomicAdd(gc + lo, 1ull); atomicAdd(gc + hi, ~0ull); }
	}
	const bool um = (flag & 4u) != 0, pm = (flag & 1u) && !(flag & 4u) && !(flag & 8u);
	/* the insert size and NM of a mapped record */
	int64_t nm = 0;
	if (mapped && ok) {
		if (pm) {
			const int32_t is = (int32_t)x[8];
			int64_t a = is < 0 ? -(int64_t)is : (int64_t)is;
			if (a >= (int64_t)T.n_isize) a = (int64_t)T.n_isize - 1;
			if (a > 0 || x[1] == x[6]) {
				const int64_t d = (int64_t)(int32_t)x[7] - (int64_t)(int32_t)x[2];
				const int sf = (flag & 0x40u) ? 1 : -1, sw = fwd ? 1 : -1, sm = (flag & 0x20u) ? -1 : 1, sd = d > 0 ? 1 : d < 0 ? -1 : 0;
				int which = -1;   /* 0 inward, 1 outward, 2 other */
				if (sw * sm > 0) which = 2;
				else if (sf * sd > 0) which = sf * sw > 0 ? 0 : 1;
				else if (sf * sd < 0) which = sf * sw > 0 ? 1 : 0;
				if (which >= 0) atomicAdd(T.isz + (int64_t)which * T.n_isize + a, 1ull);
			}
		}
		/* the aux area: an unknown type, a Z / H without its NUL, a B without its five bytes and a value cut short end the walk; so does the first NM */
		const uint64_t e = bs; uint64_t a = aux0;
		bool go = a + 3 <= e;
		while (go) {
			const uint8_t t0 = body[a], t1 = body[a + 1], ty = body[a + 2];
			a += 3;
			uint64_t sz = 0; bool stop = false;
			if (ty == 'A' || ty == 'c' || ty == 'C') sz = 1;
			else if (ty == 's' || ty == 'S') sz = 2;
			else if (ty == 'i' || ty == 'I' || ty == 'f') sz = 4;
			else if (ty == 'Z' || ty == 'H') {
				uint64_t q = a;
				while (q < e && body[q] != 0) ++q;
				stop = q >= e;
				sz = q - a + 1;
			} else if (ty == 'B') {
				stop = a + 5 > e;
				if (!stop) {
					const uint8_t st = body[a]; const uint64_t cnt = stats_ld32(body + a + 1);
					sz = 5 + ((st == 'c' || st == 'C') ? 1u : (st == 's' || st == 'S') ? 2u : 4u) * cnt;
				}
			} else stop = true;
			stop = stop || a + sz > e;
			if (!stop && t0 == 'N' && t1 == 'M') {
				if (ty == 'c') nm = (int64_t)(int8_t)body[a];
				else if (ty == 'C') nm = (int64_t)body[a];
				else if (ty == 's') nm = (int64_t)(int16_t)((uint32_t)body[a] | (uint32_t)body[a + 1] << 8);
				else if (ty == 'S') nm = (int64_t)((uint32_t)body[a] | (uint32_t)body[a + 1] << 8);
				else if (ty == 'i' || ty == 'I') nm = (int64_t)(int32_t)stats_ld32(body + a);
				stop = true;
			}
			a += sz;
			go = !stop && a + 3 <= e;
		}
	}
	const bool cover = mapped && ok && nc > 0 && !bad_cycle;
	if (act) {
		cls[i] = kept ? 1 : 0;
		stats_pb_t d; d.seq = (uint64_t)(seq - chunk); d.ls = count ? ls : 0u; d.fl = (last ? 1u : 0u) | (fwd ? 0u : 2u);
		pb[i] = d; use[i] = cover ? 1 : 0; idx[i] = (uint32_t)i;
	}
	/* the scalars: one atomic per wave each */
	stats_count(T.sc, SSG_ST_FILTERED, act && fit && !pass);
	stats_count(T.sc, SSG_ST_SECONDARY, kept && (flag & 0x100u));
	stats_count(T.sc, SSG_ST_DUP, far && (flag & 0x400u));
	stats_sum(T.sc, SSG_ST_DUP_LEN, far && (flag & 0x400u) ? ls : 0u);
	stats_sum(T.sc, SSG_ST_TOTAL_LEN, count ? ls : 0u);
	stats_count(T.sc, SSG_ST_QCFAIL, count && (flag & 0x200u));
	stats_count(T.sc, SSG_ST_PAIRED, count && (flag & 1u));
	stats_count(T.sc, SSG_ST_FIRST, count && !last);
	stats_count(T.sc, SSG_ST_LAST, count && last);
	stats_count(T.sc, SSG_ST_UNMAPPED, count && um);
	stats_sum(T.sc, SSG_ST_BASES_MAPPED, count && !um ? ls : 0u);
	stats_count(T.sc, SSG_ST_MQ0, count && !um && mapq == 0);
	stats_count(T.sc, SSG_ST_SINGLE, count && !um && !pm);
	stats_count(T.sc, SSG_ST_PAIRED_MAPPED, count && pm);
	stats_count(T.sc, SSG_ST_PROPER, count && pm && (flag & 2u));
	stats_count(T.sc, SSG_ST_ANOMALOUS, count && pm && x[1] != x[6]);
	stats_sum(T.sc, SSG_ST_MISMATCHES, (unsigned long long)nm);
	stats_sum(T.sc, SSG_ST_BASES_CIGAR, mapped && ok ? (unsigned long long)mi : 0ull);
	const int wmax = wv_max(ok ? (int)unclipped : 0), pmax = wv_max(count ? (int)ls : 0);
	if (wv_lane() == 0) {
		if (wmax > 0) atomicMax(T.sc + SSG_ST_MAX_LEN, (unsigned long long)wmax);
		if (pmax > 0) atomicMax(err + STATS_PUSH_MAX, (unsigned long long)pmax);
	}
}

__global__ void __launch_bounds__(256) ssg_k_stats_bases(const uint8_t *chunk, const stats_pb_t *pb, int64_t n_rec, int32_t tile, int64_t slab, int32_t n_tiles, stats_tab_t T)
{
	__shared__ uint32_t s_q[2 * STATS_TILE_MAX * STATS_QROW];
	__shared__ uint32_t s_b[STATS_TILE_MAX * STATS_BROW];
	for (int k = (int)threadIdx.x; k < 2 * STATS_TILE_MAX * STATS_QROW; k += 256) s_q[k] = 0;
	for (int k = (int)threadIdx.x; k < STATS_TILE_MAX * STATS_BROW; k += 256) s_b[k] = 0;
	__syncthreads();
	const int32_t t = (int32_t)(blockIdx.x % (uint32_t)n_tiles); const int64_t sl = (int64_t)(blockIdx.x / (uint32_t)n_tiles);
	const int32_t c0 = t * tile;
	const int half = (int)(threadIdx.x >> 5), j = (int)(threadIdx.x & 31);
	const uint32_t c = (uint32_t)(c0 + j);
	const bool tile_ok = tile >= 1 && tile <= STATS_TILE_MAX, on = tile_ok && j < tile;
	const int64_t r0 = sl * slab, r1 = r0 + slab < n_rec ? r0 + slab : n_rec;
	unsigned long long sumq = 0; uint32_t maxq = 0;
	for (int64_t r = r0 + half; r < r1; r += 8) {
		const stats_pb_t d = pb[r];
		if (on && c < d.ls) {
			const uint32_t b = (d.fl & 2u) ? d.ls - 1u - c : c;   /* the base and the quality byte of cycle c */
			const uint8_t *const seq = chunk + d.seq;
			const uint32_t q = seq[((uint64_t)d.ls + 1u) / 2u + b], nib = (uint32_t)(seq[b >> 1] >> ((~b & 1u) << 2)) & 15u;
			const uint32_t what = nib == 1u ? 0u : nib == 2u ? 1u : nib == 4u ? 2u : nib == 8u ? 3u : nib == 15u ? 4u : 5u;
			atomicAdd(&s_q[((d.fl & 1u) * STATS_TILE_MAX + (uint32_t)j) * STATS_QROW + q], 1u);
			atomicAdd(&s_b[(uint32_t)j * STATS_BROW + what], 1u);
			sumq += q; maxq = q > maxq ? q : maxq;
		}
	}
	__syncthreads();
	const int32_t n_q = tile_ok ? 2 * tile * 256 : 0, n_b = tile_ok ? tile * 6 : 0;
	for (int32_t k = (int32_t)threadIdx.x; k < n_q; k += 256) {
		const int32_t f = k / (tile * 256), rem = k % (tile * 256), jj = rem >> 8, q = rem & 255;
		const uint32_t v = s_q[(f * STATS_TILE_MAX + jj) * STATS_QROW + q];
		const int64_t row = (int64_t)c0 + jj;
		if (v && row < T.rows) atomicAdd(T.quals + ((int64_t)f * T.rows + row) * 256 + q, (unsigned long long)v);
	}
	for (int32_t k = (int32_t)threadIdx.x; k < n_b; k += 256) {
		const int32_t jj = k / 6, w = k % 6;
		const uint32_t v = s_b[jj * STATS_BROW + w];
		const int64_t row = (int64_t)c0 + jj;
		if (v && row < T.rows) atomicAdd(T.bases + row * 6 + w, (unsigned long long)v);
	}
	stats_sum(T.sc, SSG_ST_SUM_QUAL, sumq);
	const int wq = wv_max((int)maxq);
	if (wv_lane() == 0 && wq > 0) atomicMax(T.sc + SSG_ST_MAX_QUAL, (unsigned long long)wq);
}

/* zlib's crc32(0, p, n) with the tables in LDS */
SSG_DEVFN uint32_t stats_crc(const uint32_t *tab, const uint8_t *p, uint64_t n)
{
	uint32_t c = 0xffffffffu; uint64_t k = 0;
	for (; k + 4 <= n; k += 4) c = bzf_crc_word(tab, c, stats_ld32(p + k));
	for (; k < n; ++k) c = bzf_crc_byte(tab, c, p[k]);
	return c ^ 0xffffffffu;
}
__global__ void __launch_bounds__(256) ssg_k_stats_crc(const uint8_t *chunk, const uint64_t *loc, const uint8_t *cls, int64_t n_rec, unsigned long long *sc)
{
	__shared__ uint32_t tab[4 * 256];
	for (int k = (int)threadIdx.x; k < 4 * 256; k += 256) tab[k] = bzf_tabs.t[k >> 8][k & 255];
	__syncthreads();
	const int64_t i = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
	const bool act = i < n_rec && (cls[i] & 1);
	uint32_t cn = 0, cs = 0, cq = 0;
	if (act) {
		const uint8_t *rec = chunk + (loc[i] & STATS_OFF_MASK);
		uint32_t x[6]; memcpy(x, rec, 24);
		const uint32_t lq = x[3] & 0xffu, nc = x[4] & 0xffffu, ls = x[5];
		const uint8_t *name = rec + 36, *seq = name + lq + 4 * (uint64_t)nc;
		uint32_t nl = 0;
		while (nl < lq && name[nl] != 0) ++nl;
		cn = stats_crc(tab, name, nl);
		if (ls > 0) { const uint64_t nb = ((uint64_t)ls + 1u) / 2u; cs = stats_crc(tab, seq, nb); cq = stats_crc(tab, seq + nb, nb); }
	}
	const uint32_t sn = stats_wave_sum32(cn), ss = stats_wave_sum32(cs), sq = stats_wave_sum32(cq);
	if (wv_lane() == 0) {
		if (sn) atomicAdd(sc + SSG_ST_CHK_NAMES, (unsigned long long)sn);
		if (ss) atomicAdd(sc + SSG_ST_CHK_READS, (unsigned long long)ss);
		if (sq) atomicAdd(sc + SSG_ST_CHK_QUALS, (unsigned long long)sq);
	}
}

/* the key of a covered record: tid and pos, both taken unsigned */
SSG_DEVFN uint64_t stats_key(const uint8_t *rec) { uint32_t x[3]; memcpy(x, rec, 12); return (uint64_t)x[1] << 32 | (uint64_t)x[2]; }
__global__ void __launch_bounds__(256) ssg_k_stats_ckeys(const uint8_t *chunk, const uint64_t *loc, const uint32_t *kept, int64_t m, uint64_t last_key, int32_t have_last,
                                                         uint64_t *ckey, unsigned long long *cnt)
{
	const int64_t j = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
	const bool act = j < m;
	uint64_t k1 = 0, k0 = 0;
	if (act) {
		k1 = stats_key(chunk + (loc[kept[j]] & STATS_OFF_MASK));
		k0 = j > 0 ? stats_key(chunk + (loc[kept[j - 1]] & STATS_OFF_MASK)) : have_last ? last_key : k1;
		ckey[j] = k1;
	}
	const unsigned long long b = wv_ballot(act && k1 < k0);
	if (wv_lane() == 0 && b) atomicAdd(cnt, (unsigned long long)__popcll(b));
}

/* records kept[j0 .. j1) into the window that begins at win_beg: diff[] has n_arr entries */
__global__ void __launch_bounds__(256) ssg_k_stats_cov_add(const uint8_t *chunk, const uint64_t *loc, const uint32_t *kept, int64_t j0, int64_t j1, int64_t win_beg, int64_t n_arr, uint32_t *diff)
{
	const int64_t j = j0 + (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
	if (j >= j1) return;
	uint32_t x[6]; memcpy(x, chunk + (loc[kept[j]] & STATS_OFF_MASK), 24);
	const int64_t a = (int64_t)x[2] - win_beg, b = a + (int64_t)x[5];
	if (a >= 0 && b > a && b < n_arr) { atomicAdd(diff + a, 1u); atomicAdd(diff + b, 0xffffffffu); }
}

/* ex[p + 1]: the depth of the window's position p, p < n */
__global__ void __launch_bounds__(256) ssg_k_stats_cov_hist(const uint32_t *ex, int64_t n, int32_t cov_min, int32_t cov_max, int32_t cov_step, int32_t n_cov, unsigned long long *cov)
{
	__shared__ uint32_t s_bin[STATS_COV_MAX];
	for (int k = (int)threadIdx.x; k < STATS_COV_MAX; k += 256) s_bin[k] = 0;
	__syncthreads();
	for (int64_t p = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
		const int64_t d = (int64_t)ex[p + 1];
		if (d != 0) {
			const int64_t b = d < cov_min ? 0 : d > cov_max ? (int64_t)n_cov - 1 : 1 + (d - cov_min) / cov_step;   /* coverage_idx */
			if (b >= 0 && b < n_cov && b < STATS_COV_MAX) atomicAdd(&s_bin[b], 1u);
		}
	}
	__syncthreads();
	for (int k = (int)threadIdx.x; k < n_cov && k < STATS_COV_MAX; k += 256) { const uint32_t v = s_bin[k]; if (v) atomicAdd(cov + k, (unsigned long long)v); }
}

/* the window moved on by span positions: out[0] the depth at its new first position, out[k] the old differences behind it; n_arr + 1 entries */
__global__ void __launch_bounds__(256) ssg_k_stats_cov_carry(const uint32_t *ex, const uint32_t *diff, int64_t span, int64_t n_arr, uint32_t *out)
{
	const int64_t k = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
	if (k > n_arr) return;
	uint32_t v = 0;
	if (k == 0) v = ex[span + 1];
	else if (span + k < n_arr) v = diff[span + k];
	out[k] = v;
}
#endif
