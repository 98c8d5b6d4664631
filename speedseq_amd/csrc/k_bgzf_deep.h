/*
 * k_bgzf_deep.h -- BGZF deflate on the device at levels 7-9: the parse of k_bgzf.h with a chained match finder (zlib's `prev' chains, deflate.c
 * longest_match), for the caller who asks for a smaller file and pays for it in kernel time.  The contract is ssg_k_bgzf_deflate's: one wave per block,
 * payload / cut / n_blocks in, one raw RFC 1951 stream (a single final block, stored when it would not shrink) at tmp + b * BZ_OUT_STRIDE, its length in size[b].
 * Stages 2 and 3 (the three codes; sizes, placement, bits) are those of k_bgzf.h, restated: that kernel's machine code is pinned and stays as it is.
 *
 * The match finder.  ssg_k_bgzf_deflate looks at six candidates per position (the four newest positions of the hash's bucket inside the region, the two
 * newest before it) in no particular order of distance.  Here every position q of the block has a link prev[q]: the nearest earlier position whose next
 * four bytes have the same hash (0xffff: none).  A parse walks the links from its position -- nearest first, every earlier position of the block
 * within reach -- compares the first four bytes before it measures, and stops at the depth the level sets, at a distance above 32768, at the chain's
 * end, or when the match already reaches the end of the lane's chunk.  It keeps the longest match (the nearest among equals), tries the byte just
 * behind for runs, and applies one step of lazy evaluation, as k_bgzf.h does.
 *
 * How the links are made.  The block goes by in regions of 4 KB as in k_bgzf.h (lane l parses chunk l; a match ends inside its chunk).  Before a region is
 * parsed the wave takes its positions 64 at a time, lane l the l-th of them: the hashes of the 64 go through LDS, a lane finds the nearest lower lane
 * with its hash (64 compares on registers) or, if there is none, takes head[hash], the newest position of that hash before the group; the highest
 * lane of every hash then enters its position into head[].  That is the order a sequential insert gives, without a sort of (hash, position) pairs
 * and without anything that depends on which lane runs first: the links, and with them the stream, are the same on every run and in the host
 * emulation.  prev[] of the region being parsed lives in LDS, prev[] of the earlier regions in 128 KB of scratch per block in HBM (read only
 * for candidates before the region: lines that were written once and never read before).
 *
 * Bounds.  A link is followed only if it is below the position it came from (so a corrupt link ends the walk, and the walk cannot cycle); a position
 * enters a chain only if four bytes can be read there (q + 4 <= n), and a candidate lies below a position of that kind, so its four bytes are
 * inside the payload; match_len reads [p, p + maxl) with p + maxl <= the chunk's end <= n, and the candidate's bytes lie below those.  prev_g is
 * indexed by a 16-bit value (0x10000 entries per block), prev_l by c - r0 with r0 <= c <= p < r0 + 4096, head by BZD_HBITS bits.
 *
 * LDS: 8 KB head[] + 8 KB prev_l[] + 128 B of the group's hashes + 3.2 KB of counters, lengths and codes; the code builder's work arrays (5.8 KB)
 * lie over head[], which is dead by then.  Depths per level (BZD_DEPTH_*), chosen from profiles/r11_bgzf_levels.json; resources the compiler reports for gfx950: DESIGN.md section 6.2.
 */
#ifndef SSG_K_BGZF_DEEP_H
#define SSG_K_BGZF_DEEP_H
#define BZ_HELPERS_ONLY   /* bz_len_code, bz_dist_code, bz_code_lengths, bz_codes, bz_writer_t and the BZ_* constants; not the kernels */
#include "k_bgzf.h"

#ifndef BZD_HBITS
#define BZD_HBITS 12              /* head[]: the newest position per hash of the next four bytes */
#endif
#define BZD_REGION (64 * BZ_CHUNK)
#define BZD_NONE 0xffffu          /* no link / no hash: positions are below BZ_MAX_PAYLOAD = 0xff00 */
#define BZD_PREV_STRIDE 0x10000   /* uint16_t entries of link scratch per block */
/* candidates looked at per position at levels 7 / 8 / 9.  Each doubling buys 0.004-0.007 of the payload on a sorted BAM and costs 1.6-1.8 times the kernel time (depth 2 .. 1024
 * measured on the MI355X, 1 .. 4096 on the emulation: profiles/r11_bgzf_levels.json); with these, 4096 BAM-shaped blocks take 49 / 132 / 368 ms against ssg_k_bgzf_deflate's 35 ms and the
 * sorted BAM comes to 0.281 / 0.272 / 0.267 of its size against 0.319 (zlib level 6: 0.255).  Tried and not taken: 4 / 16 / 64 and 2 / 256 / 1024. */
#ifndef BZD_DEPTH_7
#define BZD_DEPTH_7 8
#define BZD_DEPTH_8 32
#define BZD_DEPTH_9 128
#endif

__global__ void __launch_bounds__(64) ssg_k_bgzf_deflate_deep(const uint8_t *payload, const uint64_t *cut, int n_blocks, uint8_t *tmp, uint32_t *sym, uint32_t *size, uint16_t *prev_all, int depth)
{
	__shared__ uint32_t lz_pool[(1 << BZD_HBITS) / 2];
	uint16_t *const head = (uint16_t*)lz_pool;
	static_assert(sizeof(lz_pool) >= (288 + 576 + 576) * 4, "the code builder's work arrays fit the head table's space");
	int32_t *const w_idx = (int32_t*)lz_pool; uint32_t *const w_wt = lz_pool + 288; int32_t *const w_par = (int32_t*)lz_pool + 288 + 576;
	__shared__ uint16_t prev_l[BZD_REGION];
	__shared__ uint16_t hq[64];
	__shared__ uint32_t f_ll[288], f_d[32], f_cl[19];
	__shared__ uint8_t l_ll[288], l_d[32], l_cl[19];
	__shared__ uint16_t c_ll[288], c_d[32], c_cl[19];
	__shared__ uint16_t rle[320];            /* the code-length sequence: symbol | extra value << 5 */
	__shared__ uint32_t sh_misc[8];          /* 0: n_rle, 1: hlit, 2: hdist, 3: hclen, 4: header bits */
	const int b = (int)blockIdx.x, lane = wv_lane();
	if (b >= n_blocks) return;
	const uint8_t *src = payload + cut[b];
	const int n = (int)(cut[b + 1] - cut[b]);
	uint32_t *const out = (uint32_t*)(tmp + (size_t)b * BZ_OUT_STRIDE);
	uint32_t *const my_sym = sym + (size_t)b * BZ_STRETCH_CAP * 64 + lane;
	uint16_t *const prev_g = prev_all + (size_t)b * BZD_PREV_STRIDE;
	for (int k = lane; k < (1 << BZD_HBITS) / 2; k += 64) lz_pool[k] = 0xffffffffu;
	for (int k = lane; k < 288; k += 64) f_ll[k] = 0;
	if (lane < 32) f_d[lane] = 0;
	if (lane < 19) f_cl[lane] = 0;
	for (int k = lane; k < BZ_OUT_STRIDE / 4; k += 64) out[k] = 0;
	ssg_wave_ldssync();
	/* ---- 1. LZ77 ---- */
	const int n_regions = (n + BZD_REGION - 1) / BZD_REGION;
	if (depth < 1) depth = 1;
	int ns = 0, s1 = 0, r0 = 0;
	uint16_t chunk_syms[BZ_MAX_REGIONS];
	auto match_len = [&](const int cand, const int p, const int maxl) -> int {
		int l = 0;
		while (l + 4 <= maxl && bz_load32(src + cand + l) == bz_load32(src + p + l)) l += 4;
		while (l < maxl && src[cand + l] == src[p + l]) ++l;
		return l;
	};
	/* the link of position c (c <= the position being parsed, which lies in the region that starts at r0) */
	auto link = [&](const int c) -> int { return c >= r0 ? (int)prev_l[(c - r0) & (BZD_REGION - 1)] : (int)prev_g[c & (BZD_PREV_STRIDE - 1)]; };
	/* the longest match at position p: the byte just behind (runs), then the chain of p's hash, nearest first */
	auto find = [&](const int p, int &mlen, int &mdist) {
		mlen = 0; mdist = 0;
		const int maxl = s1 - p < 258 ? s1 - p : 258;
		if (p > 0 && maxl >= 4) { const int l = match_len(p - 1, p, maxl); if (l >= 4) { mlen = l; mdist = 1; } }
		if (p + 4 > n || maxl < 4) return;
		const uint32_t wp = bz_load32(src + p);
		int last = p, c = link(p), left = depth;
		bool go = c < last && p - c <= 32768 && mlen < maxl;   /* (BZD_NONE is above every position) */
		while (go) {   /* per-lane trip count: one flag, one exit test */
			const uint32_t wc = bz_load32(src + c); const int nx = link(c);   /* the candidate's bytes and its link: one round trip, not two */
			if (wc == wp) {
				const int l = match_len(c, p, maxl);
				if (l > mlen) { mlen = l; mdist = p - c; }
			}
			last = c; c = nx; --left;
			go = left > 0 && c < last && p - c <= 32768 && mlen < maxl;
		}
	};
	auto literal = [&](const int p) { const uint32_t c = src[p]; atomicAdd(&f_ll[c], 1u); my_sym[(size_t)ns * 64] = c; ++ns; };
	SSG_UNROLL for (int j = 0; j < BZ_MAX_REGIONS; ++j) {
		const int ns0 = ns;
		if (j < n_regions) {
			r0 = j * BZD_REGION;
			/* the region's links, 64 positions at a time in the order of the positions (wave-uniform trip counts) */
			const int n_groups = ((n - r0 < BZD_REGION ? n - r0 : BZD_REGION) + 63) / 64;
			for (int g = 0; g < n_groups; ++g) {
				const int k = g * 64 + lane, q = r0 + k;
				const uint32_t h = q + 4 <= n ? (bz_load32(src + q) * 2654435761u) >> (32 - BZD_HBITS) : BZD_NONE;
				hq[lane] = (uint16_t)h;
				ssg_wave_ldssync();
				uint32_t m_lo = 0, m_hi = 0;   /* the lanes of the group with this lane's hash */
				for (int t = 0; t < 32; ++t) { m_lo |= (uint32_t)((uint32_t)hq[t] == h) << t; m_hi |= (uint32_t)((uint32_t)hq[32 + t] == h) << t; }
				const unsigned long long m = (unsigned long long)m_hi << 32 | m_lo, below = m & ((1ull << lane) - 1ull);
				const int near = below ? 63 - __clzll(below) : -1;
				const bool later = (m >> lane) >> 1 != 0;
				uint32_t pv = BZD_NONE;
				if (h != BZD_NONE) pv = near >= 0 ? (uint32_t)(q - lane + near) : (uint32_t)head[h];
				prev_l[k] = (uint16_t)pv; prev_g[q] = (uint16_t)pv;   /* q <= r0 + 4095 <= 0xffff */
				ssg_wave_ldssync();   /* every lane has read head[] and hq[] */
				if (h != BZD_NONE && !later) head[h] = (uint16_t)q;
				ssg_wave_ldssync();
			}
			ssg_wave_memsync();   /* the links in HBM are read by other lanes when later regions are parsed */
			const int c0 = r0 + lane * BZ_CHUNK, s0 = c0 < n ? c0 : n;
			s1 = s0 + BZ_CHUNK < n ? s0 + BZ_CHUNK : n;
			for (int pos = s0; pos < s1; ) {
				int mlen, mdist;
				find(pos, mlen, mdist);
				if (mlen && mlen < s1 - pos && pos + 1 < s1) {   /* one step of lazy matching: a longer match one byte on is worth a literal */
					int l2, d2;
					find(pos + 1, l2, d2);
					if (l2 > mlen + 1) { literal(pos); ++pos; mlen = l2; mdist = d2; }
				}
				if (mlen) {
					int lc, le, lv, dc, de, dv;
					bz_len_code(mlen, lc, le, lv); bz_dist_code(mdist, dc, de, dv);
					atomicAdd(&f_ll[257 + lc], 1u); atomicAdd(&f_d[dc], 1u);
					my_sym[(size_t)ns * 64] = 0x80000000u | (uint32_t)mlen << 16 | (uint32_t)(mdist - 1); ++ns;
					pos += mlen;
				} else { literal(pos); ++pos; }
			}
			ssg_wave_ldssync();   /* prev_l is rewritten for the next region */
		}
		chunk_syms[j] = (uint16_t)(ns - ns0);
	}
	ssg_wave_ldssync();
	/* ---- 2. the three codes, by one lane (k_bgzf.h) ---- */
	if (lane == 0) {
		f_ll[256] = 1;   /* end of block */
		bz_code_lengths(f_ll, 286, 15, l_ll, w_idx, w_wt, w_par);
		bz_code_lengths(f_d, 30, 15, l_d, w_idx, w_wt, w_par);
		int hlit = 286; while (hlit > 257 && l_ll[hlit - 1] == 0) --hlit;
		int hdist = 30; while (hdist > 1 && l_d[hdist - 1] == 0) --hdist;
		/* run-length form of the two length sequences (RFC 1951 3.2.7: 16 = repeat previous 3-6, 17 = 3-10 zeros, 18 = 11-138 zeros) */
		int nr = 0;
		for (int t = 0; t < 2; ++t) {
			const uint8_t *L = t ? l_d : l_ll; const int cnt = t ? hdist : hlit;
			for (int i = 0; i < cnt; ) {
				const int v = L[i]; int run = 1;
				while (i + run < cnt && L[i + run] == v) ++run;
				i += run;
				if (v == 0) {
					while (run >= 11) { const int r = run < 138 ? run : 138; rle[nr++] = (uint16_t)(18 | (r - 11) << 5); run -= r; }
					if (run >= 3) { rle[nr++] = (uint16_t)(17 | (run - 3) << 5); run = 0; }
					while (run-- > 0) rle[nr++] = 0;
				} else {
					rle[nr++] = (uint16_t)v; --run;
					while (run >= 3) { const int r = run < 6 ? run : 6; rle[nr++] = (uint16_t)(16 | (r - 3) << 5); run -= r; }
					while (run-- > 0) rle[nr++] = (uint16_t)v;
				}
			}
		}
		for (int k = 0; k < nr; ++k) ++f_cl[rle[k] & 31];
		bz_code_lengths(f_cl, 19, 7, l_cl, w_idx, w_wt, w_par);
		bz_codes(l_ll, 286, 15, c_ll); bz_codes(l_d, 30, 15, c_d); bz_codes(l_cl, 19, 7, c_cl);
		const int order[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
		int hclen = 19; while (hclen > 4 && l_cl[order[hclen - 1]] == 0) --hclen;
		uint32_t hb = 3 + 5 + 5 + 4 + 3 * (uint32_t)hclen;
		for (int k = 0; k < nr; ++k) { const int s = rle[k] & 31; hb += l_cl[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0); }
		sh_misc[0] = (uint32_t)nr; sh_misc[1] = (uint32_t)hlit; sh_misc[2] = (uint32_t)hdist; sh_misc[3] = (uint32_t)hclen; sh_misc[4] = hb;
	}
	ssg_wave_ldssync();
	/* ---- 3. sizes, placement, bits (k_bgzf.h): the header, then the chunks in the order of their positions ---- */
	auto sym_bits = [&](const uint32_t s) -> uint32_t {
		if (!(s & 0x80000000u)) return l_ll[s];
		int lc, le, lv, dc, de, dv;
		bz_len_code((int)((s >> 16) & 0x1ff), lc, le, lv); bz_dist_code((int)(s & 0xffff) + 1, dc, de, dv);
		return (uint32_t)(l_ll[257 + lc] + le + l_d[dc] + de);
	};
	const uint32_t hb = sh_misc[4];
	uint32_t chunk_bit0[BZ_MAX_REGIONS], base = hb;
	{	int k = 0;
		SSG_UNROLL for (int j = 0; j < BZ_MAX_REGIONS; ++j) {
			uint32_t bits = 0;
			for (int e = k + chunk_syms[j]; k < e; ++k) bits += sym_bits(my_sym[(size_t)k * 64]);
			const uint32_t incl = (uint32_t)wv_scan_add((int)bits);
			chunk_bit0[j] = base + incl - bits;
			base += (uint32_t)wv_get((int)incl, 63);
		}
	}
	const uint32_t total_bits = base + l_ll[256];
	const uint32_t total_bytes = (total_bits + 7) >> 3;
	if (total_bytes >= (uint32_t)n + 5u) {   /* does not shrink: one stored block (RFC 1951 3.2.4) */
		uint8_t *o = (uint8_t*)out;
		if (lane == 0) { o[0] = 1; o[1] = (uint8_t)(n & 0xff); o[2] = (uint8_t)(n >> 8); o[3] = (uint8_t)~o[1]; o[4] = (uint8_t)~o[2]; }
		for (int k = lane; k < n; k += 64) o[5 + k] = src[k];
		if (lane == 0) size[b] = (uint32_t)n + 5u;
		return;
	}
	bz_writer_t w;
	if (lane == 0) {   /* block header: BFINAL = 1, BTYPE = 2, HLIT, HDIST, HCLEN, the code-length code, the two length sequences; and the end-of-block code */
		const int order[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
		bz_w_init(w, out, 0);
		bz_w_put(w, 1u | 2u << 1, 3);
		bz_w_put(w, sh_misc[1] - 257, 5); bz_w_put(w, sh_misc[2] - 1, 5); bz_w_put(w, sh_misc[3] - 4, 4);
		for (uint32_t k = 0; k < sh_misc[3]; ++k) bz_w_put(w, l_cl[order[k]], 3);
		for (uint32_t k = 0; k < sh_misc[0]; ++k) {
			const int s = rle[k] & 31, ev = rle[k] >> 5;
			bz_w_put(w, c_cl[s], l_cl[s]);
			if (s >= 16) bz_w_put(w, (uint32_t)ev, s == 16 ? 2 : s == 17 ? 3 : 7);
		}
		bz_w_end(w);
		bz_w_init(w, out, base); bz_w_put(w, c_ll[256], l_ll[256]); bz_w_end(w);
	}
	{	int k = 0;
		SSG_UNROLL for (int j = 0; j < BZ_MAX_REGIONS; ++j) if (chunk_syms[j]) {
			bz_w_init(w, out, chunk_bit0[j]);
			for (int e = k + chunk_syms[j]; k < e; ++k) {
				const uint32_t s = my_sym[(size_t)k * 64];
				if (s & 0x80000000u) {
					int lc, le, lv, dc, de, dv;
					bz_len_code((int)((s >> 16) & 0x1ff), lc, le, lv); bz_dist_code((int)(s & 0xffff) + 1, dc, de, dv);
					bz_w_put(w, c_ll[257 + lc], l_ll[257 + lc]); if (le) bz_w_put(w, (uint32_t)lv, le);
					bz_w_put(w, c_d[dc], l_d[dc]); if (de) bz_w_put(w, (uint32_t)dv, de);
				} else bz_w_put(w, c_ll[s], l_ll[s]);
			}
			bz_w_end(w);
		}
	}
	if (lane == 0) size[b] = total_bytes;
}
#endif
