/*
 * k_smem2.h -- the seeding kernel of the product path: upstream mem_collect_intv = bwt_smem1a from every
 * position the previous call returned (pass 1), bwt_smem1a with min_intv = occurrences + 1 from the middle of long SMEMs with few
 * occurrences (pass 2), bwt_seed_strategy1 (pass 3); oracle/orc_mem.c restates them from upstream bwt.c / bwamem.c.
 *
 * One lane per read; the three passes are a per-lane state machine around ONE bwt_extend site per loop iteration, so that every lane of
 * the wave that has an extension pending issues its two rank-block fetches (and the fetch of its next interval-list entry) in the same
 * memory round trip, whatever loop of the nested algorithm it is in.  A read's three passes cost ~800 dependent extensions of two random
 * 64-byte lines each; what bounds the kernel is the rate of random lines (tools/dbg/gather_probe.cpp), not streaming bandwidth.
 *
 * Control flow discipline (measured on the MI355X in round 4): the loop has ONE exit and it is wave-uniform
 * (`no lane has work'), and the extension site is one predicated block -- no divergent `break' or `continue' anywhere in the loop.  The
 * round-3 form of this kernel left the loop per lane (`if (state == FIN) break; if (pend == NONE) continue;' plus a `continue' out of the
 * middle of the site); hipcc 7.2 compiled some instances of that text into code that computes different intervals on the GPU (second-pass
 * SMEMs cut short) while the same text is right under the host emulation, and which instance went wrong depended on nothing one would
 * touch on purpose (the translation unit the kernel sat in, two unused arguments).  The uniform form of the same statements is right in
 * every build that was tried.
 *
 * Order of the passes: upstream runs bwt_seed_strategy1 (pass 3) last; here it runs FIRST.  The passes only append to the read's list, pass 2
 * reads pass 1's entries alone, and the list is sorted by (start, end) afterwards, so the order of appending is free -- and pass 3 is a plain
 * chain of ~150 extensions that never makes a read heavy: done first, its seeds survive when the read is given up in pass 1 or 2, and the
 * wave-per-read kernel, whose time is dependent round trips, does not walk that chain again.
 *
 * Per-read budget: a read whose extensions exceed `max_ext', or whose forward pass leaves a row of more than `max_row' intervals, is given up (out_n = -2, nothing of it is kept) and the caller hands it to the
 * wave-per-read kernel: a repeat-heavy read costs 10-50x the average, every one of its extensions is a dependent round trip, and a lane
 * that picked one up late used to hold the whole launch open long after the pool of reads had run dry.
 */
#ifndef SSG_K_SMEM2_H
#define SSG_K_SMEM2_H
#include "ssg_dev.h"

#define SSG_S2_QWORDS 40   /* the read as 4-bit codes, 8 per LDS word: reads up to 320 bases */
enum { S2_FWD = 0, S2_BWD, S2_P3F, S2_READ, S2_P1, S2_P2, S2_P3, S2_OUT, S2_FIN };
enum { S2_PEND_NONE = 0, S2_PEND_FWD, S2_PEND_BWD, S2_PEND_P3 };

/* interval-list entry, 16 bytes: x0, x1 < 2^40, x2 < 2^39 (an occurrence count never exceeds the text length), info = end position < 512 */
struct alignas(16) ssg_pk2_t { uint64_t w0, w1; };
SSG_DEVFN ssg_pk2_t s2_pk(const ssg_intv_t &v)
{ ssg_pk2_t p; p.w0 = v.x0 | (v.x1 & 0xffffffull) << 40; p.w1 = (v.x1 >> 24) | v.x2 << 16 | v.info << 55; return p; }
SSG_DEVFN ssg_intv_t s2_unpk(const ssg_pk2_t &p)
{ ssg_intv_t v; v.x0 = p.w0 & 0xffffffffffull; v.x1 = (p.w0 >> 40) | (p.w1 & 0xffffull) << 24; v.x2 = (p.w1 >> 16) & 0x7fffffffffull; v.info = p.w1 >> 55; return v; }
SSG_DEVFN void s2_set_intv(const ssg_index_view_t &ix, int c, ssg_intv_t &ik)
{	/* upstream bwt_set_intv */
	ik.x0 = ix.L2[c] + 1; ik.x2 = ix.L2[c+1] - ix.L2[c]; ik.x1 = ix.L2[3-c] + 1; ik.info = 0;
}

/* launch statistics of the instrumented instance (TUNE): [0] first lane started, [1] first lane that found the pool of reads empty, [2] last
 * lane done (100 MHz wall clock); [3] reads given up; [8 + b] reads whose extension count has b significant bits; [48] wave rounds,
 * [49] lanes with an extension pending, summed over rounds, [50] lanes with a read; of the given-up reads whose third pass was finished: [4] extensions of
 * passes 1 and 2 in calls of bwt_smem1a that were finished, [5] in all calls; [52 + S2_WC_*] the wave kernel's counts (tuning builds only) */
#ifdef SSG_EMU
static unsigned long long ssg_s2_stat[64];
SSG_DEVFN unsigned long long s2_wall() { return 1; }
#else
__device__ unsigned long long ssg_s2_stat[64];
SSG_DEVFN unsigned long long s2_wall() { return (unsigned long long)wall_clock64(); }
#endif
#define S2_STAT_MIN(i, v) atomicMin(&ssg_s2_stat[i], (unsigned long long)(v))
#define S2_STAT_MAX(i, v) atomicMax(&ssg_s2_stat[i], (unsigned long long)(v))
#define S2_STAT_ADD(i, v) atomicAdd(&ssg_s2_stat[i], (unsigned long long)(v))

#ifndef SSG_S2_WAVES
#define SSG_S2_WAVES 4
#endif
#ifndef SSG_S2_TRIPS
#define SSG_S2_TRIPS 2
#endif

/* ---- uniform values: every lane of the wave holds the same value; tell the compiler (scalar registers, scalar branches) ---- */
#ifdef SSG_EMU
SSG_DEVFN int wv_uni(int v) { return v; }
SSG_DEVFN uint64_t wv_uni64(uint64_t v) { return v; }
#else
SSG_DEVFN int wv_uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
SSG_DEVFN uint64_t wv_uni64(uint64_t v) { return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32; }
#endif
SSG_DEVFN ssg_intv_t wv_uni_intv(const ssg_intv_t &v) { ssg_intv_t o; o.x0 = wv_uni64(v.x0); o.x1 = wv_uni64(v.x1); o.x2 = wv_uni64(v.x2); o.info = wv_uni64(v.info); return o; }

/* what the two shared-rank forms below end with: ssg_bwt_extend1_lean's interval arithmetic from the sums of the two queries' blocks (prk / prl: nt | n1 << 16 of
 * ssg_cnt_pair for the lower / upper query) and their count quarters (ck / cl) -- on scalars where the caller's values are wave-uniform, per lane where they are not */
SSG_DEVFN ssg_intv_t s2_coop_tail(const ssg_index_view_t &ix, const ssg_intv_t &ik, const int c, const int is_back, const int prk, const int prl, const uint32_t ck[4], const uint32_t cl[4])
{
	const uint64_t kx = is_back ? ik.x0 : ik.x1, ox = is_back ? ik.x1 : ik.x0;
	const uint64_t k = kx - 1, l = k + ik.x2;
	const bool kneg = k == (uint64_t)-1, lneg = l == (uint64_t)-1;
	const uint64_t k2 = kneg ? 0 : k - (k >= ix.primary), l2 = lneg ? 0 : l - (l >= ix.primary);
	const int nbk = prk >> 16, nak = (prk & 0xffff) - nbk, nbl = prl >> 16, nal = (prl & 0xffff) - nbl;
	const uint64_t oak = ((uint64_t)ck[0] | (uint64_t)ck[1] << 32) + (uint64_t)nak, obk = ((uint64_t)ck[2] | (uint64_t)ck[3] << 32) + (uint64_t)nbk;
	const uint64_t oal = ((uint64_t)cl[0] | (uint64_t)cl[1] << 32) + (uint64_t)nal, obl = ((uint64_t)cl[2] | (uint64_t)cl[3] << 32) + (uint64_t)nbl;
	const uint64_t Tk = k2 + 1, Tl = l2 + 1;
	uint64_t tkc = (c & 1) ? obk : oak, tkg = c == 0 ? Tk - oak : c == 1 ? Tk - oak - obk : c == 2 ? obk : 0;
	uint64_t tlc = (c & 1) ? obl : oal, tlg = c == 0 ? Tl - oal : c == 1 ? Tl - oal - obl : c == 2 ? obl : 0;
	if (kneg) tkc = tkg = 0;
	if (lneg) tlc = tlg = 0;
	const uint64_t no = ox + (kx <= ix.primary && kx + ik.x2 - 1 >= ix.primary) + (tlg - tkg);
	const uint64_t nk = ix.L2[c] + 1 + tkc;
	ssg_intv_t o;
	o.x2 = tlc - tkc; o.info = 0;
	if (is_back) { o.x0 = nk; o.x1 = no; } else { o.x1 = nk; o.x0 = no; }
	return o;
}

/*
 * ssg_bwt_extend1_lean of a wave-UNIFORM interval, the rank work shared by 16 lanes (every row of 16 does the same; the result is read from the first).
 * Lanes 0-7 of the row take the eight symbol words of the lower query's block, lanes 8-15 the upper query's (in one block the two halves fetch the same
 * line); the first lane of each half also fetches the count quarter of the followed base.  Each lane masks its word to the query's position and takes the
 * two popcounts of ssg_cnt_pair packed into one register (a block's sums are at most 128 each); three DPP adds give the sums of a half, v_readlane
 * makes them and the counts scalars, and the interval arithmetic is that of ssg_bwt_extend1_lean on scalars.  Same bits as ssg_bwt_extend1_lean in every
 * word (tests/test_smem_wave_coop.py runs both on the same inputs).  All 64 lanes must call it together; c = 0..3 and is_back wave-uniform.
 */
SSG_DEVFN ssg_intv_t s2_extend_coop(const ssg_index_view_t &ix, const ssg_intv_t &ik, const int c, const int is_back)
{
	const int l16 = wv_lane() & 15, up = l16 >> 3, wi = l16 & 7;
	const uint64_t kx = is_back ? ik.x0 : ik.x1, ox = is_back ? ik.x1 : ik.x0;
	const uint64_t k = kx - 1, l = k + ik.x2;
	const bool kneg = k == (uint64_t)-1, lneg = l == (uint64_t)-1;
	const uint64_t k2 = kneg ? 0 : k - (k >= ix.primary), l2 = lneg ? 0 : l - (l >= ix.primary);   /* k2 <= l2 */
	const uint64_t q2 = up ? l2 : k2;                                  /* this lane's query */
	const uint32_t *const blk = ix.bwt + ((q2 >> 7) << 4);
	const uint32_t w = blk[8 + wi];
	ssg_q16_t cq; cq.v[0] = cq.v[1] = cq.v[2] = cq.v[3] = 0;
	if (wi == 0) cq = ((const ssg_q16_t*)blk)[c >> 1];
	/* ssg_cnt_pair's word wi: a word wholly above the position is shifted by 31 and counts nothing */
	int sh = 32 * (wi + 1) - (((int)(q2 & 127) + 1) << 1); sh = sh < 0 ? 0 : sh > 31 ? 31 : sh;
	const uint32_t hs = (((w >> 1) ^ ((c & 2) ? 0u : 0xffffffffu)) & 0x55555555u) >> sh;
	const int pr = wv_seg8_sum(__popc(hs) | __popc(hs & (w >> sh)) << 16);   /* nt | n1 << 16 */
	const int prk = wv_get(pr, 7), prl = wv_get(pr, 15);
	uint32_t ck[4], cl[4];
	SSG_UNROLL for (int i = 0; i < 4; ++i) { ck[i] = (uint32_t)wv_get((int)cq.v[i], 0); cl[i] = (uint32_t)wv_get((int)cq.v[i], 8); }
	return s2_coop_tail(ix, ik, c, is_back, prk, prl, ck, cl);
}

/* The same for FOUR intervals at once, one per row of 16 lanes (ik uniform within a row; c and is_back wave-uniform): for the short rows of the backward pass, where
 * the lane-per-entry form spends a whole wave's instructions on one to four entries.  The sums and counts stay in vector registers -- every lane of a row ends
 * with both queries' (wv_seg8_allsum, wv_xor8) and does the row's interval arithmetic; every lane returns its row's result. */
SSG_DEVFN ssg_intv_t s2_extend_coop4(const ssg_index_view_t &ix, const ssg_intv_t &ik, const int c, const int is_back)
{
	const int l16 = wv_lane() & 15, up = l16 >> 3, wi = l16 & 7;
	const uint64_t kx = is_back ? ik.x0 : ik.x1, ox = is_back ? ik.x1 : ik.x0;
	const uint64_t k = kx - 1, l = k + ik.x2;
	const bool kneg = k == (uint64_t)-1, lneg = l == (uint64_t)-1;
	const uint64_t k2 = kneg ? 0 : k - (k >= ix.primary), l2 = lneg ? 0 : l - (l >= ix.primary);
	const uint64_t q2 = up ? l2 : k2;
	const uint32_t *const blk = ix.bwt + ((q2 >> 7) << 4);
	const uint32_t w = blk[8 + wi];
	const ssg_q16_t cq = ((const ssg_q16_t*)blk)[c >> 1];          /* every lane: its half's count quarter (one line for the eight) */
	int sh = 32 * (wi + 1) - (((int)(q2 & 127) + 1) << 1); sh = sh < 0 ? 0 : sh > 31 ? 31 : sh;
	const uint32_t hs = (((w >> 1) ^ ((c & 2) ? 0u : 0xffffffffu)) & 0x55555555u) >> sh;
	const int pr = wv_seg8_allsum(__popc(hs) | __popc(hs & (w >> sh)) << 16), po = wv_xor8(pr);
	const int prk = up ? po : pr, prl = up ? pr : po;
	uint32_t ck[4], cl[4];
	SSG_UNROLL for (int i = 0; i < 4; ++i) { const uint32_t o = (uint32_t)wv_xor8((int)cq.v[i]); ck[i] = up ? o : cq.v[i]; cl[i] = up ? cq.v[i] : o; }
	return s2_coop_tail(ix, ik, c, is_back, prk, prl, ck, cl);
}

/*
 * ssg_k_smem_heavy -- one WAVE per read, for the reads the lane kernel gave up (repeat-heavy: thousands of extensions, nearly all of them
 * in the backward passes of bwt_smem1a, where every entry of a long list is extended by the same base).  The wave walks upstream's
 * nested loops as written; what is wave-wide is the inner loop of the backward pass: lane l extends entry base + l of the row, and the
 * row's survivors are appended in list order by ballot + rank.  Upstream appends a survivor when its occurrence count differs from the
 * last appended one's; along a row the counts are non-decreasing (each entry's pattern is a prefix of the one before it), so that is the
 * same as `differs from the previous survivor's'.  Of the dead entries only the row's first can be an SMEM (upstream's test on the start of
 * the call's previous SMEM fails for all the others once it was decided for the first).  The forward extensions and the third pass are
 * chains of dependent extensions with a wave-uniform interval: s2_extend_coop shares an extension's rank work among 16 lanes and keeps the interval on the scalar
 * unit, and a chain's first bases come from the table of short-pattern intervals (HISTORY.md section 14).  A backward row of at most four entries goes through
 * s2_extend_coop4, an entry per row of 16 lanes.
 * SC = list capacity (> longest read + 1), lists and the read in LDS.  ids: the reads to do (positions in the batch), n_ids on the device.
 */
SSG_DEVFN long s2_ktab_off(int j) { return (long)(((1ull << (2 * j)) - 4ull) / 3ull); }   /* table of short-pattern intervals (below): entries of the levels below j */
/* what the lane kernel leaves of a given-up read whose third pass is finished, 16 bytes: w[0] = phase (1: pass 1, 2: pass 2) | (the x, or the k, at which its unfinished
 * call of bwt_smem1a began) << 8, w[1] = the list's length at that call's start, w[2] = old_n (pass 2: the end of pass 1's entries), w[3] = the read's extensions at that call's start */
struct alignas(16) ssg_s2_resume_t { uint32_t w[4]; };
enum { S2_PATH_RESUME_P1 = 0, S2_PATH_RESUME_P2, S2_PATH_RESTART_P3, S2_PATH_P1_FROM_0, S2_PATH_N };   /* how the wave kernel took a read up (counted for the tests) */
/* launch counts of the wave kernel, tuning builds only (SSG_TUNING; ssg_s2_stat[52 + i], printed by ssg_seed_smem2 under SSG_S2_TUNE=1) */
enum { S2_WC_READS = 0, S2_WC_FWD, S2_WC_P3, S2_WC_BWD, S2_WC_ROW4, S2_WC_ROW16, S2_WC_ROW64, S2_WC_ROWMORE, S2_WC_EXT, S2_WC_TABSTART, S2_WC_TABEXT, S2_WC_N };
/* one read by the whole wave (see ssg_k_smem_heavy); qb: >= 264 bytes of LDS for the read, l0 / l1: two lists of > len + 1 entries in LDS.
 * kt_tab / kt_k: the table of short-pattern intervals as the lane kernel has it (kt_k = 0: none; else 2 <= kt_k < min_seed_len, at most 15).
 * The chains of dependent extensions (forward loop, third pass) have a wave-uniform interval: their first bases come from the table, all prefixes
 * in one round trip, and the rest goes through s2_extend_coop.  Returns the read's extension count (uniform). */
SSG_DEVFN unsigned long long s2_wave_read(const ssg_index_view_t &ix, const ssg_mem_opt_t &opt, const int split_len, const int it, const int32_t *read_ids, const uint8_t *seq, const int64_t *off,
                                          ssg_intv_t *out_intv, int32_t *out_n, const int cap, uint8_t *qb, ssg_pk2_t *l0, ssg_pk2_t *l1, const ssg_pk2_t *kt_tab, const int kt_k,
                                          const ssg_s2_resume_t *resume, unsigned int *paths)
{
	const int lane = wv_lane();
	unsigned long long nx = 0;
	unsigned int wc[S2_WC_N];
	for (int t = 0; t < S2_WC_N; ++t) wc[t] = 0;
	const int r = read_ids ? read_ids[it] : it;
	const uint8_t *q = seq + off[r];
	const int len = (int)(off[r+1] - off[r]);
	ssg_wave_ldssync();
	for (int b = lane; b < len; b += 64) qb[b] = q[b];
	ssg_wave_ldssync();
	/* the run of unambiguous bases from position b, at most kt_k of them and never past the read's end, and their table code (first base lowest) */
	auto kt_run = [&](const int b, uint32_t &code) -> int {
		const int qc = lane < kt_k && b + lane < len ? (int)qb[b + lane] : 4;
		const int run = __ffsll(wv_ballot(qc > 3)) - 1;     /* lanes kt_k .. 63 always vote: kt_k <= 15 */
		code = (uint32_t)wv_sum(lane < run ? (qc & 3) << (2 * lane) : 0);
		return run;
	};
	ssg_intv_t *const mem = out_intv + (long)it * cap;
	/* what the lane kernel left: out_n = -2: nothing; -3 - k: the third pass is done, its k seeds are the list's first entries (k <= cap: it would have reported an overflow otherwise) */
	const int left = -2 - out_n[it];
	const bool skip_p3 = left >= 1;
	const int n_p3 = skip_p3 ? left - 1 : 0;
	int mem_n = n_p3, ovf = 0;
	/* where the lane kernel's unfinished call began: resume there with the lists as they were at its start (no record: everything but a finished third pass again) */
	int phase = 1, x0 = 0, k0 = n_p3, old_n_rec = 0;
	if (skip_p3 && resume) {
		const ssg_s2_resume_t rec = resume[it];
		const int w0 = wv_uni((int)rec.w[0]);
		phase = w0 & 255; mem_n = wv_uni((int)rec.w[1]); old_n_rec = wv_uni((int)rec.w[2]);
		if (phase == 1) x0 = w0 >> 8; else k0 = w0 >> 8;
	}
	if (paths && lane == 0) atomicAdd(&paths[!skip_p3 ? S2_PATH_RESTART_P3 : phase == 2 ? S2_PATH_RESUME_P2 : x0 > 0 ? S2_PATH_RESUME_P1 : S2_PATH_P1_FROM_0], 1u);
	/* one call of upstream bwt_smem1a (max_intv = 0): start sx, smallest occurrence count min_intv; returns where the next call starts */
	auto smem1 = [&](const int sx, uint64_t min_intv) -> int {
		if (min_intv < 1) min_intv = 1;
		ssg_intv_t ik;
		int n = 0, i = sx + 1;
		bool stop = false;
		uint32_t code = 0;
		const int run = kt_k >= 2 ? kt_run(sx, code) : 0;
		if (run >= 2) {
			/* the first run - 1 extensions from the table, one round trip: lane j = 1 .. run has E_j, the interval of the first j bases, and (j >= 2) stands for
			 * upstream's extension from j - 1 to j bases: E_(j-1) is pushed where the occurrence count changes, and the chain stops at the first change below min_intv */
			const bool has = lane >= 1 && lane <= run, ext = lane >= 2 && lane <= run;
			const int jl = has ? lane : 1;
			ssg_pk2_t e; e.w0 = e.w1 = 0;
			if (has) e = kt_tab[s2_ktab_off(jl) + (long)(code & ((1u << (2 * jl)) - 1u))];
			ssg_intv_t ev = s2_unpk(e);
			const uint64_t px2 = (uint64_t)(uint32_t)wv_prev((int)(uint32_t)ev.x2, 0) | (uint64_t)(uint32_t)wv_prev((int)(uint32_t)(ev.x2 >> 32), 0) << 32;   /* x2 of E_(j-1) */
			const unsigned long long stopm = wv_ballot(ext && ev.x2 != px2 && ev.x2 < min_intv);
			const int jstop = stopm ? __ffsll(stopm) - 1 : run + 1;
			const unsigned long long pm = wv_ballot(ext && lane <= jstop && ev.x2 != px2) >> 1;   /* bit l: lane l pushes E_l */
			if (pm >> lane & 1) { ev.info = (uint64_t)(sx + lane); l0[__popcll(pm & ((1ull << lane) - 1ull))] = s2_pk(ev); }
			n = __popcll(pm);
			stop = stopm != 0;
			const int src = stop ? jstop - 1 : run;   /* stopped: ik stays the last pushed */
			nx += (unsigned long long)((stop ? jstop : run) - 1);
			ssg_pk2_t u; u.w0 = (uint64_t)wv_get64((long long)e.w0, src); u.w1 = (uint64_t)wv_get64((long long)e.w1, src);
			ik = s2_unpk(u); ik.info = (uint64_t)(sx + src); i = sx + src;
			if (SSG_TUNING) { ++wc[S2_WC_TABSTART]; wc[S2_WC_TABEXT] += (unsigned int)((stop ? jstop : run) - 1); }
		} else { s2_set_intv(ix, wv_uni((int)qb[sx]), ik); ik.info = (uint64_t)(sx + 1); }
		while (!stop && i < len) {   /* forward: the intervals of [sx, i) at every change of the occurrence count, shortest first */
			const int cq = wv_uni((int)qb[i]);
			if (cq < 4) {
				const ssg_intv_t ok = s2_extend_coop(ix, ik, 3 - cq, 0); ++nx;
				if (SSG_TUNING) ++wc[S2_WC_FWD];
				if (ok.x2 != ik.x2) { l0[n++] = s2_pk(ik); stop = ok.x2 < min_intv; }
				if (!stop) { ik = ok; ik.info = (uint64_t)(i + 1); ++i; }
			} else { l0[n++] = s2_pk(ik); stop = true; }
		}
		if (!stop) l0[n++] = s2_pk(ik);
		const int ret = (int)ik.info;
		int cur = 0, prev_n = n, rev = 1, m1_n = 0, m1_last_beg = 0;
		bool more = true;
		for (int ib = sx - 1; more && ib >= -1; --ib) {   /* backward: every interval of the row by the base left of it */
			const int cb = ib < 0 ? -1 : wv_uni((int)qb[ib]) < 4 ? wv_uni((int)qb[ib]) : -1;
			int curr_n = 0; bool have_last = false; uint64_t last_x2 = 0;
			ssg_wave_ldssync();
			for (int base = 0; base < prev_n; base += 64) {
				const int jj = base + lane; const bool valid = jj < prev_n;
				ssg_intv_t p; p.x0 = p.x1 = p.x2 = p.info = 0;
				if (valid) p = s2_unpk((cur ? l1 : l0)[rev ? prev_n - 1 - jj : jj]);
				ssg_intv_t okc; okc.x0 = okc.x1 = okc.x2 = okc.info = 0;
				if (cb >= 0 && prev_n <= 4) {
					/* a row of at most four entries: entry g by the lanes 16 g .. 16 g + 15 (a row of lanes without an entry does the first again), the
					 * results back to lanes 0 .. 3, where the row's bookkeeping below expects them */
					const int g = lane >> 4, ge = g < prev_n ? g : 0;
					const ssg_intv_t og = s2_extend_coop4(ix, s2_unpk((cur ? l1 : l0)[rev ? prev_n - 1 - ge : ge]), cb, 1);
					const int src = (lane & 3) << 4;
					const uint64_t g0 = (uint64_t)wv_bcast64((long long)og.x0, src), g1 = (uint64_t)wv_bcast64((long long)og.x1, src), g2 = (uint64_t)wv_bcast64((long long)og.x2, src);
					if (valid) { okc.x0 = g0; okc.x1 = g1; okc.x2 = g2; }
				} else if (valid && cb >= 0) okc = ssg_bwt_extend1_lean(ix, p, cb, 1);
				if (cb >= 0) nx += (unsigned long long)(prev_n - base < 64 ? prev_n - base : 64);
				if (SSG_TUNING && cb >= 0) { ++wc[S2_WC_BWD]; ++wc[prev_n <= 4 ? S2_WC_ROW4 : prev_n <= 16 ? S2_WC_ROW16 : prev_n <= 64 ? S2_WC_ROW64 : S2_WC_ROWMORE]; }
				const bool alive = valid && cb >= 0 && okc.x2 >= min_intv;
				if (base == 0 && !wv_get((int)alive, 0)) {   /* the row's first entry dies here: an SMEM if it starts left of the call's previous one */
					const int beg = ib + 1;
					if (m1_n == 0 || beg < m1_last_beg) {
						++m1_n; m1_last_beg = beg;
						const int end0 = wv_get((int)(uint32_t)p.info, 0);
						if (end0 - beg >= opt.min_seed_len) {
							if (mem_n < cap) { if (lane == 0) { ssg_intv_t o = p; o.info |= (uint64_t)beg << 32; mem[mem_n] = o; } } else ovf = 1;
							++mem_n;
						}
					}
				}
				const unsigned long long am = wv_ballot(alive);
				if (am) {
					const unsigned long long below = am & ((1ull << lane) - 1ull);
					const int pl = below ? 63 - __clzll(below) : 0;
					const uint64_t px2 = (uint64_t)wv_shfl64_xor((long long)okc.x2, lane ^ pl);   /* okc.x2 of lane pl */
					const bool push = alive && (below ? okc.x2 != px2 : (!have_last || okc.x2 != last_x2));
					const unsigned long long pm = wv_ballot(push);
					if (push) { ssg_intv_t o = okc; o.info = p.info; (cur ? l0 : l1)[curr_n + __popcll(pm & ((1ull << lane) - 1ull))] = s2_pk(o); }
					curr_n += __popcll(pm);
					have_last = true; last_x2 = (uint64_t)wv_get64((long long)okc.x2, 63 - __clzll(am));
				}
			}
			if (curr_n == 0) more = false;
			else { cur ^= 1; rev = 0; prev_n = curr_n; }
		}
		ssg_wave_ldssync();
		return ret;
	};
	if (len >= opt.min_seed_len) {
		int x = phase == 1 ? x0 : len;
		while (x < len) { if (wv_uni((int)qb[x]) < 4) x = smem1(x, 1); else ++x; }   /* pass 1 (resumed in pass 2: done) */
		const int old_n = phase == 1 ? (mem_n < cap ? mem_n : cap) : old_n_rec;
		ssg_wave_memsync();
		for (int k = k0; k < old_n; ++k) {   /* pass 2: re-seed from the middle of long SMEMs with few occurrences */
			const ssg_intv_t m = wv_uni_intv(mem[k]);
			const int start = (int)(m.info >> 32), end = (int)(uint32_t)m.info;
			if (end - start >= split_len && m.x2 <= (uint64_t)opt.split_width) {
				const int sx = (start + end) >> 1;
				if (wv_uni((int)qb[sx]) < 4) (void)smem1(sx, m.x2 + 1);
			}
		}
		if (opt.max_mem_intv > 0 && !skip_p3) {   /* pass 3: upstream bwt_seed_strategy1 from every position it returns */
			x = 0;
			while (x < len) {
				if (wv_uni((int)qb[x]) > 3) ++x;
				else {
					/* with the table the chain starts kt_k bases in (upstream records nothing before the pattern has min_seed_len > kt_k bases), and a start
					 * with an ambiguous base or the read's end inside the window moves past it as upstream's loop returns: what S2_P3START does in the lane kernel */
					ssg_intv_t ik;
					int i = x + 1, nxt = len; bool stop = false;
					uint32_t code = 0;
					const int run = kt_k >= 2 ? kt_run(x, code) : 0;
					if (kt_k >= 2 && run < kt_k) { nx += (unsigned long long)(run - 1); nxt = x + run >= len ? len : x + run + 1; stop = true; ik.x0 = ik.x1 = ik.x2 = ik.info = 0; }
					else if (kt_k >= 2) {
						const ssg_pk2_t e = kt_tab[s2_ktab_off(kt_k) + (long)code];
						ssg_pk2_t u; u.w0 = wv_uni64(e.w0); u.w1 = wv_uni64(e.w1);
						ik = s2_unpk(u); i = x + kt_k; nx += (unsigned long long)(kt_k - 1);
						if (SSG_TUNING) { ++wc[S2_WC_TABSTART]; wc[S2_WC_TABEXT] += (unsigned int)(kt_k - 1); }
					} else s2_set_intv(ix, wv_uni((int)qb[x]), ik);
					while (!stop && i < len) {
						const int cq = wv_uni((int)qb[i]);
						if (cq < 4) {
							const ssg_intv_t ok = s2_extend_coop(ix, ik, 3 - cq, 0); ++nx;
							if (SSG_TUNING) ++wc[S2_WC_P3];
							if (ok.x2 < (uint64_t)opt.max_mem_intv && i - x >= opt.min_seed_len) {
								if (ok.x2 > 0) {
									if (mem_n < cap) { if (lane == 0) { ssg_intv_t o = ok; o.info = (uint64_t)x << 32 | (uint64_t)(i + 1); mem[mem_n] = o; } } else ovf = 1;
									++mem_n;
								}
								nxt = i + 1; stop = true;
							} else { ik = ok; ++i; }
						} else { nxt = i + 1; stop = true; }
					}
					x = nxt;
				}
			}
		}
	}
	if (lane == 0) out_n[it] = ovf ? -1 : mem_n;
	if (SSG_TUNING && lane == 0) {
		wc[S2_WC_READS] = 1;
		for (int t = 0; t < S2_WC_N; ++t) if (t != S2_WC_EXT && wc[t]) S2_STAT_ADD(52 + t, wc[t]);
		S2_STAT_ADD(52 + S2_WC_EXT, nx);
	}
	return nx;
}

/* ---- table of the intervals of all short patterns (ssg_index.ktab) ----
 * The bidirectional interval of a pattern does not depend on the order in which the pattern was extended to, so the intervals of ALL patterns
 * of 1..K bases can be tabulated once per index: 16 bytes each (x0, x1, x2 in 40 bits), level j (4^j entries, little-endian base-4 pattern
 * code: first base least significant) after the levels below it -- 1.4 GB for K = 13 on a human-size index (built in ~20 ms), 22.9 GB for the K = 15 of ssg_seed.cpp.  A bwt_extend
 * whose RESULT pattern has at most K bases then is one 16-byte load at an address that depends only on the read, instead of two rank blocks
 * (2.5 loads each) and the popcounts; roughly four extensions in ten of a 150-base read are that short. */
/* (s2_ktab_off, the entries of the levels below j, stands above the wave kernel, which uses it too) */
/* level j from level j - 1: the four one-base left extensions of every pattern by upstream's own bwt_extend (is_back = 1): an entry is bit for
 * bit what the extension it stands in for returns.  Children of pattern code p are 4p .. 4p + 3. */
__global__ void ssg_k_ktab_level(ssg_index_view_t ix, int j, ssg_pk2_t *tab)
{
	const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= (1L << (2 * (j - 1)))) return;
	ssg_pk2_t *const out = tab + s2_ktab_off(j) + 4 * p;
	ssg_intv_t ok[4];
	if (j == 1) { for (int c = 0; c < 4; ++c) s2_set_intv(ix, c, ok[c]); }
	else ssg_bwt_extend(ix, s2_unpk(tab[s2_ktab_off(j - 1) + p]), ok, 1);
	for (int c = 0; c < 4; ++c) { ok[c].info = 0; out[c] = s2_pk(ok[c]); }
}
/* self-check (SSG_KTAB_VERIFY=1): every `stride'-th pattern of level j once more, the way the seeding kernel reaches it without the table --
 * from its first base by forward extensions with the kernel's own ssg_bwt_extend1_lean -- and compared */
__global__ void ssg_k_ktab_verify(ssg_index_view_t ix, int j, long stride, const ssg_pk2_t *tab, unsigned long long *bad)
{
	const long t = (long)blockIdx.x * blockDim.x + threadIdx.x, code = t * stride;
	if (code >= (1L << (2 * j))) return;
	ssg_intv_t ik;
	s2_set_intv(ix, (int)(code & 3), ik);
	for (int k = 1; k < j; ++k) ik = ssg_bwt_extend1_lean(ix, ik, 3 - (int)((code >> (2 * k)) & 3), 0);
	const ssg_intv_t e = s2_unpk(tab[s2_ktab_off(j) + code]);
	if (ik.x2 != e.x2 || (ik.x2 && (ik.x0 != e.x0 || ik.x1 != e.x1))) atomicAdd(&bad[j], 1ull);
}
/* the 16 codes from position b of a read held as 4-bit codes, 8 per LDS word (word w of the read at qw[w * stride]), first base lowest */
SSG_DEVFN uint64_t s2_window(const uint32_t *qw, int stride, int b)
{
	const int w0 = b >> 3, sh = (b & 7) << 2;
	const int w1 = w0 + 1 < SSG_S2_QWORDS ? w0 + 1 : SSG_S2_QWORDS - 1, w2 = w0 + 2 < SSG_S2_QWORDS ? w0 + 2 : SSG_S2_QWORDS - 1;
	uint64_t v = ((uint64_t)qw[w0 * stride] | (uint64_t)qw[w1 * stride] << 32) >> sh;
	if (sh) v |= (uint64_t)qw[w2 * stride] << (64 - sh);
	return v;
}
/* table code of the n <= 15 unambiguous bases from position b */
SSG_DEVFN uint32_t s2_code(const uint32_t *qw, int stride, int b, int n)
{
	uint64_t v = s2_window(qw, stride, b);
	v &= 0x3333333333333333ull; v = (v | v >> 2) & 0x0f0f0f0f0f0f0f0full; v = (v | v >> 4) & 0x00ff00ff00ff00ffull;
	v = (v | v >> 8) & 0x0000ffff0000ffffull; v = (v | v >> 16) & 0xffffffffull;
	return (uint32_t)v & ((1u << (2 * n)) - 1u);
}

/*
 * seq: concatenated nt4 codes, off[r]..off[r+1] delimit read r.  out_intv: [n_reads x cap]; out_n: per-read interval count (-1: the
 * per-read capacity or a work list overflowed; -2: given up; -3 - k: given up with the k seeds of the finished third pass in place).  scratch: per launched wave 2 lists x scap entries x
 * 64 lanes of 16 bytes, entry e of lane l at [e * 64 + l] (lanes pushing their e-th entries together write one 1-KB span).
 * next_read: shared counter the lanes take their reads from (evens out the per-read cost).  n_ext_read (optional): extensions per read.
 * heavy_ids / n_heavy (optional): the given-up reads, appended in no particular order, for ssg_k_smem_heavy (launched behind this kernel).
 */
template <bool TUNE, bool KT>
__global__ void __launch_bounds__(64, SSG_S2_WAVES) ssg_k_smem2(ssg_index_view_t ix, ssg_mem_opt_t opt, int n_reads, const int32_t *read_ids,
                           const uint8_t *seq, const int64_t *off, ssg_intv_t *out_intv, int32_t *out_n, int cap,
                           ssg_pk2_t *scratch, int scap, unsigned long long *n_extend, unsigned int *next_read, unsigned int max_ext, int max_row, uint32_t *n_ext_read, int32_t *heavy_ids, unsigned int *n_heavy,
                           const ssg_pk2_t *kt_tab, int kt_k /* KT: the table of short-pattern intervals, kt_k < min_seed_len */,
                           ssg_s2_resume_t *resume /* per read (position in the batch), written for the given-up ones whose third pass is finished; only with a budget, else NULL */)
{
	__shared__ uint32_t qlds[SSG_S2_QWORDS * 64];
	const long gt = (long)blockIdx.x * blockDim.x + threadIdx.x;
	const int lane = (int)(threadIdx.x & 63);
	ssg_pk2_t *const vec0 = scratch + (gt >> 6) * 2 * scap * 64 + lane, *const vec1 = vec0 + (long)scap * 64;
	const uint32_t *const ql_ = qlds + lane;
#define S2Q(i) ((int)((ql_[((i) >> 3) * 64] >> (((i) & 7) << 2)) & 15u))
#define S2V(v, e) ((v)[(long)(e) * 64])
	const int split_len = (int)(opt.min_seed_len * opt.split_factor + .499);
	unsigned long long my_nx = 0;
	unsigned int rd_nx = 0, nx_p3 = 0;   /* extensions of the current read; of its third pass */
	unsigned int nx_call = 0; int mem_call = 0;   /* when the current call of bwt_smem1a began: the read's extensions, its list's length (for the resume record) */
#define S2_CALL() do { nx_call = rd_nx; mem_call = mem_n; } while (0)
	long it = 0;
	int state = S2_READ, pend = S2_PEND_NONE;
	int len = 0, x = 0, k = 0, old_n = 0, caller = 0, mem_n = 0, ovf = 0, heavy = 0, n_p3 = -1;   /* n_p3 < 0: the third pass is not finished */
	ssg_intv_t *mem = 0;
	int sx = 0, i = 0, j = 0, curr_n = 0, prev_n = 0, prev_rev = 0, flip = 0, m1_n = 0, m1_last_beg = 0, ret = 0, e_c = 0;
	uint64_t min_intv = 1, last_x2 = 0;
	ssg_intv_t ik, p;
	ik.x0 = ik.x1 = ik.x2 = ik.info = 0; p = ik;
	ssg_pk2_t pn, c0, first; pn.w0 = pn.w1 = 0; c0 = first = pn;
	if (TUNE) S2_STAT_MIN(0, s2_wall());
	/* transitions done where they arise (no state of their own):
	 * the forward list becomes `prev', walked from its top (= ik), ret = end of the longest match; return of bwt_smem1a to its caller */
#define S2_FWDEND() do { ret = (int)ik.info; flip ^= 1; prev_n = curr_n < scap ? curr_n : scap; prev_rev = 1; curr_n = 0; i = sx - 1; j = 0; first = s2_pk(ik); state = S2_BWD; if (prev_n > max_row) { heavy = 1; state = S2_OUT; } } while (0)
	/* next start of the third pass (upstream bwt_seed_strategy1 from every position): skip ambiguous bases, open the interval */
#define S2_P3END() do { n_p3 = mem_n; nx_p3 = rd_nx; x = 0; state = S2_P1; } while (0)   /* the third pass runs FIRST here (see the kernel's comment): on to pass 1 */
/* With the table the first kt_k - 1 extensions of a start collapse into one look-up: upstream records nothing before the pattern has min_seed_len
 * (> kt_k) bases, so only an ambiguous base or the read's end inside the window matters -- the start then moves past it exactly as upstream's
 * loop returns, one window per trip (state S2_P3 comes back here); the skipped bwt_extend calls still count as the algorithm's. */
#define S2_P3START() do { \
		while (x < len && S2Q(x) > 3) ++x; \
		if (x >= len) S2_P3END(); \
		else if (!KT || kt_k < 2) { s2_set_intv(ix, S2Q(x), ik); i = x + 1; state = S2_P3F; } \
		else { \
			const unsigned long long nm_ = s2_window(ql_, 64, x) & 0x4444444444444444ull; \
			int run_ = nm_ ? (int)((__ffsll(nm_) - 1) >> 2) : 16; \
			run_ = run_ > len - x ? len - x : run_; \
			if (run_ >= kt_k) { ik = s2_unpk(kt_tab[s2_ktab_off(kt_k) + (long)s2_code(ql_, 64, x, kt_k)]); i = x + kt_k; my_nx += (unsigned long long)(kt_k - 1); rd_nx += (unsigned int)(kt_k - 1); state = S2_P3F; } \
			else { my_nx += (unsigned long long)(run_ - 1); rd_nx += (unsigned int)(run_ - 1); if (x + run_ >= len) S2_P3END(); else { x += run_ + 1; state = S2_P3; } } \
		} \
	} while (0)
#define S2_RET() do { if (caller == 1) { x = ret; state = S2_P1; } else { ++k; state = S2_P2; } } while (0)
	/* an SMEM leaves the backward pass: upstream keeps it when it starts left of the previous one of the call; the caller's length filter applied here */
#define S2_EMIT(pp, beg) do { if (m1_n == 0 || (beg) < m1_last_beg) { ++m1_n; m1_last_beg = (beg); \
		if ((int)(uint32_t)(pp).info - (beg) >= opt.min_seed_len) { ssg_intv_t o_ = (pp); o_.info |= (uint64_t)(beg) << 32; if (mem_n < cap) mem[mem_n] = o_; else ovf = 1; ++mem_n; } } } while (0)
	for (;;) {
		/* a bounded number of state-machine steps per extension round: a lane in the middle of a transition sits the round out instead of
		 * making the whole wave walk through the dispatch again */
		/* (a trip after the first is skipped by the whole wave when no lane is in a transition: 52.4 -> 51.4 ms) */
		SSG_UNROLL for (int trip = 0; trip < SSG_S2_TRIPS; ++trip) if ((trip == 0 || wv_ballot(pend == S2_PEND_NONE && state != S2_FIN)) && pend == S2_PEND_NONE && state != S2_FIN) {
			ssg_pk2_t *const curr = flip ? vec1 : vec0;
			if (state == S2_FWD) { /* top of upstream's forward loop: for (i = x + 1; i < len; ++i) */
				if (i < len && S2Q(i) < 4) { pend = S2_PEND_FWD; e_c = 3 - S2Q(i); }
				else { if (curr_n < scap) S2V(curr, curr_n) = s2_pk(ik); else ovf = 1; ++curr_n; S2_FWDEND(); }
			} else if (state == S2_BWD) { /* for (i = x - 1; i >= -1; --i) for (j = 0; j < prev->n; ++j) */
				if (j >= prev_n) {
					bool back_to_caller = curr_n == 0;
					if (!back_to_caller) { flip ^= 1; prev_n = curr_n < scap ? curr_n : scap; prev_rev = 0; curr_n = 0; j = 0; --i; first = c0; back_to_caller = i < -1; }
					if (back_to_caller) S2_RET();
				} else {
					p = s2_unpk(j == 0 ? first : pn);
					const int cb = i < 0 ? -1 : S2Q(i) < 4 ? S2Q(i) : -1;
					if (cb >= 0) { pend = S2_PEND_BWD; e_c = cb; }
					else { /* no base to extend with: only the first (longest) interval of the row can be an SMEM, the rest are no-ops */
						if (j == 0) S2_EMIT(p, i + 1);
						j = prev_n;
					}
				}
			} else if (state == S2_P3F) {
				if (i >= len) S2_P3END();
				else if (S2Q(i) < 4) { pend = S2_PEND_P3; e_c = 3 - S2Q(i); }
				else { x = i + 1; S2_P3START(); }
			} else if (state == S2_READ) {
				it = (long)atomicAdd(next_read, 1u);
				if (it >= n_reads) { state = S2_FIN; if (TUNE) S2_STAT_MIN(1, s2_wall()); }
				else {
					const int r = read_ids ? read_ids[it] : (int)it;
					const uint8_t *q = seq + off[r];
					len = (int)(off[r+1] - off[r]);
					mem = out_intv + (long)it * cap; mem_n = 0; ovf = 0; rd_nx = 0; nx_p3 = 0; heavy = 0;
					/* the read as 4-bit codes, 8 per LDS word, fetched as aligned 8-byte words, four LDS words per round trip (this runs with few lanes active) */
					const unsigned al = (unsigned)((uintptr_t)q & 7), sh8 = al << 3;
					const uint64_t *const qa = (const uint64_t*)(q - al);
					const int nw = (len + 7) >> 3, nb = (int)al + len;   /* nb: bytes from qa to the read's end */
					for (int w0 = 0; w0 < nw; w0 += 4) {
						uint64_t t[5];
						SSG_UNROLL for (int jj = 0; jj < 5; ++jj) t[jj] = (w0 + jj) * 8 < nb ? qa[w0 + jj] : 0;
						SSG_UNROLL for (int jj = 0; jj < 4; ++jj) {
							const int w = w0 + jj;
							if (w < nw) {
								uint64_t v = sh8 ? (t[jj] >> sh8) | (t[jj + 1] << (64 - sh8)) : t[jj];
								v &= 0x0f0f0f0f0f0f0f0full;
								v = (v | v >> 4) & 0x00ff00ff00ff00ffull;
								v = (v | v >> 8) & 0x0000ffff0000ffffull;
								uint32_t v32 = (uint32_t)(v | v >> 16);
								const int nv = len - w * 8;
								if (nv < 8) v32 &= (1u << (nv << 2)) - 1u;
								qlds[w * 64 + lane] = v32;
							}
						}
					}
					x = 0;
					n_p3 = opt.max_mem_intv > 0 ? -1 : 0;
					state = len < opt.min_seed_len ? S2_OUT : opt.max_mem_intv > 0 ? S2_P3 : S2_P1;
				}
			} else if (state == S2_P1) {
				if (x >= len) { old_n = mem_n < cap ? mem_n : cap; k = n_p3 > 0 ? n_p3 : 0; state = S2_P2; }
				else if (S2Q(x) > 3) ++x;
				else { S2_CALL(); sx = x; min_intv = 1; caller = 1; state = S2_FWD; m1_n = 0; curr_n = 0; i = sx + 1; s2_set_intv(ix, S2Q(sx), ik); ik.info = (uint64_t)(sx + 1); }
			} else if (state == S2_P2) { /* re-seed from the middle of long SMEMs with few occurrences */
				if (k >= old_n) state = S2_OUT;
				else {
					const ssg_intv_t m = mem[k];
					const int start = (int)(m.info >> 32), end = (int)(uint32_t)m.info;
					if (end - start < split_len || m.x2 > (uint64_t)opt.split_width) ++k;
					else {
						S2_CALL();
						sx = (start + end) >> 1; min_intv = m.x2 + 1; caller = 2; m1_n = 0; curr_n = 0; i = sx + 1;
						if (S2Q(sx) > 3) S2_RET();   /* bwt_smem1a returns at once on an ambiguous base */
						else { s2_set_intv(ix, S2Q(sx), ik); ik.info = (uint64_t)(sx + 1); state = S2_FWD; }
					}
				}
			} else if (state == S2_P3) {
				S2_P3START();
			} else { /* S2_OUT */
				const bool given_up = heavy != 0;
				out_n[it] = ovf ? -1 : given_up ? (n_p3 < 0 ? -2 : -3 - n_p3) : mem_n;   /* given up: the seeds of a finished third pass (the list's first n_p3 entries) stay */
				if (given_up && !ovf && heavy_ids) heavy_ids[atomicAdd(n_heavy, 1u)] = (int32_t)it;
				/* a given-up read whose third pass is finished leaves where its unfinished call began: the wave kernel resumes there (the entries that call
				 * emitted are dropped: the list is cut back to its length at the call's start).  No extension since the third pass ended: no call has done
				 * anything yet (`caller' may still be the previous read's), pass 1 from the read's start */
				const bool fresh = rd_nx == nx_p3;
				if (given_up && n_p3 >= 0 && resume) {
					ssg_s2_resume_t rec_;
					rec_.w[0] = fresh ? 1u : (unsigned int)caller | (unsigned int)(caller == 1 ? sx : k) << 8;
					rec_.w[1] = (unsigned int)(fresh ? n_p3 : mem_call); rec_.w[2] = (unsigned int)old_n; rec_.w[3] = fresh ? rd_nx : nx_call;
					resume[it] = rec_;
				}
				/* n_extend counts the algorithm's extensions (upstream's own count): the wave kernel counts what it does of this read -- all of it, or from the unfinished call on */
				if (given_up) my_nx -= n_p3 < 0 || !resume ? (n_p3 < 0 ? rd_nx : rd_nx - nx_p3) : fresh ? 0u : rd_nx - nx_call;
				if (n_ext_read) n_ext_read[it] = rd_nx;
				if (TUNE) { S2_STAT_ADD(8 + (64 - __clzll((unsigned long long)(rd_nx | 1u))), 1); if (given_up) S2_STAT_ADD(3, 1); }
#if SSG_TUNING
				if (TUNE && given_up && n_p3 >= 0) { S2_STAT_ADD(4, nx_call - nx_p3); S2_STAT_ADD(5, rd_nx - nx_p3); }   /* what the wave kernel does again: in calls that were finished; in all */
#endif
				state = S2_READ;
			}
		}
		if (TUNE) { const unsigned long long rdy = wv_ballot(pend != S2_PEND_NONE), alv = wv_ballot(state != S2_FIN); if (lane == 0) { S2_STAT_ADD(48, 1); S2_STAT_ADD(49, __popcll(rdy)); S2_STAT_ADD(50, __popcll(alv)); } }
		if (!wv_ballot(state != S2_FIN)) break;   /* the only exit: no lane of the wave has work */
		/* the pattern an extension ends with: [i, end of p) going left, [start, i] going right; up to kt_k bases its interval is in the table.  The two
		 * ways are separate passes for the wave and each is skipped when no lane wants it (the ballots stand where every lane passes) */
		const int pat_b = pend == S2_PEND_BWD ? i : pend == S2_PEND_FWD ? sx : x, pat_n = (pend == S2_PEND_BWD ? (int)p.info : i + 1) - pat_b;
		const bool by_table = KT && pend != S2_PEND_NONE && pat_n <= kt_k;
		const bool any_tab = KT && wv_ballot(by_table) != 0, any_ext = !KT || wv_ballot(pend != S2_PEND_NONE && !by_table) != 0;
		if (pend != S2_PEND_NONE) {
			/* ---- the one extension site: the rank-block quarters of both queries + the next list entry, one memory round trip ---- */
			const ssg_pk2_t *const prev = flip ? vec0 : vec1;
			ssg_pk2_t *const curr = flip ? vec1 : vec0;
			const bool back = pend == S2_PEND_BWD;
			const int jn = back && j + 1 < prev_n ? j + 1 : 0;
			ssg_pk2_t pf; pf.w0 = pf.w1 = 0;
			if (jn) pf = S2V(prev, prev_rev ? prev_n - 1 - jn : jn);   /* issued together with the rank-block loads below */
			ssg_intv_t okc; okc.x0 = okc.x1 = okc.x2 = okc.info = 0;
			if (any_tab) { if (by_table) okc = s2_unpk(kt_tab[s2_ktab_off(pat_n) + (long)s2_code(ql_, 64, pat_b, pat_n)]); }
			if (any_ext) { if (!by_table) okc = ssg_bwt_extend1_lean(ix, back ? p : ik, e_c, back); }
			++my_nx; ++rd_nx;
			if (pend == S2_PEND_FWD) {
				bool fwd_end = false;
				if (okc.x2 != ik.x2) {
					if (curr_n < scap) S2V(curr, curr_n) = s2_pk(ik); else ovf = 1;
					++curr_n;
					if (okc.x2 < min_intv) { S2_FWDEND(); fwd_end = true; }   /* upstream's break: ik stays the last pushed */
				}
				if (!fwd_end) { ik = okc; ik.info = (uint64_t)(i + 1); ++i; }
			} else if (back) {
				pn = pf;
				if (okc.x2 < min_intv) { if (curr_n == 0) S2_EMIT(p, i + 1); }
				else if (curr_n == 0 || okc.x2 != last_x2) {
					ssg_intv_t o = okc; o.info = p.info;
					const ssg_pk2_t po = s2_pk(o);
					if (curr_n == 0) c0 = po;
					if (curr_n < scap) S2V(curr, curr_n) = po; else ovf = 1;
					++curr_n; last_x2 = okc.x2;
				}
				++j;
			} else { /* S2_PEND_P3 */
				if (okc.x2 < (uint64_t)opt.max_mem_intv && i - x >= opt.min_seed_len) {
					if (okc.x2 > 0) { ssg_intv_t o = okc; o.info = (uint64_t)x << 32 | (uint64_t)(i + 1); if (mem_n < cap) mem[mem_n] = o; else ovf = 1; ++mem_n; }
					x = i + 1; S2_P3START();
				} else { ik = okc; ++i; }
			}
			pend = S2_PEND_NONE;
			if (rd_nx > max_ext) { heavy = 1; state = S2_OUT; }   /* given up: the wave-per-read kernel takes the read from its start */
		}
	}
	if (TUNE) S2_STAT_MAX(2, s2_wall());
#undef S2Q
#undef S2V
#undef S2_FWDEND
#undef S2_P3START
#undef S2_P3END
#undef S2_RET
#undef S2_EMIT
#undef S2_CALL
	if (n_extend && my_nx) atomicAdd(n_extend, my_nx);
}

#ifdef SSG_HEAVY_MIN_WAVES   /* variant builds: tools/dbg/seed_variants.sh */
#define SSG_HEAVY_BOUNDS __launch_bounds__(64, SSG_HEAVY_MIN_WAVES)
#else
#define SSG_HEAVY_BOUNDS __launch_bounds__(64)
#endif
template <int SC>
__global__ void SSG_HEAVY_BOUNDS ssg_k_smem_heavy(ssg_index_view_t ix, ssg_mem_opt_t opt, const int32_t *ids, const unsigned int *n_ids, const int32_t *read_ids,
                           const uint8_t *seq, const int64_t *off, ssg_intv_t *out_intv, int32_t *out_n, int cap, unsigned long long *n_extend, unsigned int *next,
                           const ssg_pk2_t *kt_tab, int kt_k /* the table of short-pattern intervals as ssg_k_smem2 has it; kt_k = 0: none */,
                           const ssg_s2_resume_t *resume /* the lane kernel's records, per read */, unsigned int *paths /* S2_PATH_* counters, or NULL */)
{
	__shared__ uint8_t qb[328];
	__shared__ ssg_pk2_t lst[2][SC];
	const int split_len = (int)(opt.min_seed_len * opt.split_factor + .499);
	const int n_todo = (int)*n_ids;
	unsigned long long nx = 0;
	for (;;) {
		const long t = wv_queue_pop(next);
		if (t >= n_todo) break;
		nx += s2_wave_read(ix, opt, split_len, ids[t], read_ids, seq, off, out_intv, out_n, cap, qb, lst[0], lst[1], kt_tab, kt_k, resume, paths);
	}
	if (n_extend && nx && wv_lane() == 0) atomicAdd(n_extend, nx);
}
/* self-check of the denser table (SSG_SA_VERIFY=1): every `stride`-th entry against upstream's own bwt_sa walk on the file's samples */
__global__ void ssg_k_sa_verify(ssg_index_view_t ix, int new_intv, const uint64_t *sa_new, long n_new, long stride, unsigned long long *bad)
{
	const long j = ((long)blockIdx.x * blockDim.x + threadIdx.x) * stride;
	if (j >= n_new) return;
	const uint64_t r = (uint64_t)j * (uint64_t)new_intv;
	const uint64_t want = (r % (uint64_t)ix.sa_intv) == 0 ? ix.sa[r / (uint64_t)ix.sa_intv] : ssg_bwt_sa(ix, r);
	if (sa_new[j] != want) atomicAdd(bad, 1ull);
}
#endif
