/*
 * k_mswkeys.h -- mate rescue's list logic on compact keys (upstream mem_matesw after its alignments are known).
 *
 * Every window of a listed pair has been aligned ahead of the decision (k_mswlane.h), so what is left of mem_matesw is bookkeeping: the skip test, the
 * insertion of the rescued hit, mem_sort_dedup_patch.  ssg_k_matesw (k_pair.h) does it on the 88-byte records in HBM -- a scan, a shift of the list's tail
 * and two passes of the re-sort per window, each a dependent round trip of the wave.  Only six fields of a record take part in any decision, so here the list
 * being rescued into is a VIEW: the 32-byte keys (ssg_sdp_key_t) of its records, indexed by the record's position in the read's slice, and the list order as
 * an array of 16-bit positions.  The view lives in the wave's LDS up to SSG_SDP_CAP positions and in a per-wave HBM slab for lists of up to SSG_SDP_BIG entries.
 *   load       one pass over the records of the side (six fields each)
 *   skip test  on the keys
 *   window     from its slot only (state 2, or state 1 where ksw_align2 has no reverse pass); there is no Smith-Waterman code in this unit
 *   hit        the record is appended ONCE in the slice's head-room (position nrec, past n_reg); its key goes to key[nrec], its position into the order before
 *              the first lower-scoring entry: 2-byte entries move, no record does
 *   re-sort    wv_sort_dedup_incr's rules (k_sdp.h) on the view when the list is a fixed point of the scan, the key-based full sort of
 *              wv_sort_dedup_fast otherwise; dropped regions leave the order only
 *   end        when both sides are decided, the records of a list that changed are gathered once by position and written with n_reg
 * n_comp: every re-sort that does anything sets n_comp = 1 in all survivors, and a hit is always re-sorted in the window that recorded it, so "all survivors
 * carry n_comp = 1" is one flag per list (the exception, a list of one record that the full sort returns untouched, leaves the flag alone).
 *
 * Nothing a later step of ssg_k_matesw would read is written before the pair is decided (head-room past n_reg is scratch), so the kernel may give a pair
 * up at any point: it goes to a leftover list, with its slot bases, and ssg_k_matesw replays it from the start.  Reasons (SSG_MK_WHY_*): a window without a
 * slot or without the reverse pass it needs; a tie the incremental scan cannot order; no head-room; a list of more than SSG_SDP_BIG entries; anything that would
 * set an error code.  Counters are added for decided pairs only, so the two kernels' sums are what ssg_k_matesw alone would count.
 */
#ifndef SSG_K_MSWKEYS_H
#define SSG_K_MSWKEYS_H
#include "k_sw.h"        /* SSG_KSW_*, ssg_align2_has_rev: device functions only */
#include "k_sdp.h"
#include "k_mswslot.h"

#define SSG_MK_WAVES 4      /* waves per workgroup */
#define SSG_MK_ANCH 64      /* anchors a side (upstream's b[i]); more is ssg_k_matesw's error 3 */
enum { SSG_MK_WHY_SLOT = 1, SSG_MK_WHY_REV = 2, SSG_MK_WHY_TIE = 3, SSG_MK_WHY_ROOM = 4, SSG_MK_WHY_BIG = 5, SSG_MK_WHY_ERR = 6, SSG_MK_NWHY = 7 };
/* counters (unsigned int): [0] pairs left over (the length of the leftover list), [1] pairs decided here, [1 + why] pairs left over by reason,
 * [1 + SSG_MK_NWHY] windows of the pairs decided here */
#define SSG_MK_NCNT (2 + SSG_MK_NWHY)

struct ssg_mk_lds_t { ssg_sdp_key_t key[SSG_SDP_CAP]; uint64_t skey[SSG_SDP_CAP]; uint16_t ord[SSG_SDP_CAP], alt[SSG_SDP_CAP], keep[SSG_SDP_CAP]; int64_t arb[2][SSG_MK_ANCH]; int32_t arid[2][SSG_MK_ANCH]; };
#define SSG_MK_BIGCAP (SSG_SDP_BIG + 256)   /* positions of the slab: a list of SSG_SDP_BIG entries and the hits recorded into it (4 an anchor, at most SSG_MK_ANCH anchors) */
struct ssg_mk_big_t { ssg_sdp_key_t key[SSG_MK_BIGCAP]; uint64_t skey[SSG_MK_BIGCAP]; uint16_t ord[SSG_MK_BIGCAP], alt[SSG_MK_BIGCAP], keep[SSG_MK_BIGCAP]; };
/* the view of one list (wave-uniform): key[] by record position, ord[0 .. n) = the list, alt[] = the other order buffer, nrec = first free position */
struct ssg_mk_view_t { ssg_sdp_key_t *key; uint64_t *skey; uint16_t *ord, *alt; int n, nrec, big; };

SSG_DEVFN void mk_load(ssg_mk_view_t &v, ssg_mk_lds_t *L, ssg_mk_big_t *B, const ssg_alnreg_t *a, int an)
{
	v.big = an > SSG_SDP_CAP;
	if (v.big) { v.key = B->key; v.skey = B->skey; v.ord = B->ord; v.alt = B->alt; }
	else { v.key = L->key; v.skey = L->skey; v.ord = L->ord; v.alt = L->alt; }
	v.n = v.nrec = an;
	ssg_wave_memsync();
	for (int i = wv_lane(); i < an; i += 64) {
		const ssg_alnreg_t *r = &a[i];
		ssg_sdp_key_t k; k.re = r->re; k.rb = r->rb; k.qb = r->qb; k.qe = r->qe; k.score = r->score; k.rid = r->rid;
		v.key[i] = k; v.ord[i] = (uint16_t)i;
	}
	ssg_wave_memsync();
}
/* LDS -> slab, when a position beyond SSG_SDP_CAP is needed */
SSG_DEVFN void mk_to_big(ssg_mk_view_t &v, ssg_mk_big_t *B)
{
	ssg_wave_memsync();
	for (int i = wv_lane(); i < v.nrec; i += 64) B->key[i] = v.key[i];
	for (int i = wv_lane(); i < v.n; i += 64) B->ord[i] = v.ord[i];
	ssg_wave_memsync();
	v.key = B->key; v.skey = B->skey; v.ord = B->ord; v.alt = B->alt; v.big = 1;
}
/* the hit's key at position nrec, its position into the order before the first lower-scoring entry (mem_matesw); returns where.  Needs nrec below the
 * arrays' capacity (the caller moves the view or gives up first). */
SSG_DEVFN int mk_insert(ssg_mk_view_t &v, const ssg_sdp_key_t &kb)
{
	const int lane = wv_lane(), n = v.n;
	ssg_wave_memsync();
	int t2 = n;
	for (int k = lane; k < n; k += 64) if (v.key[v.ord[k]].score < kb.score) { t2 = k; break; }
	t2 = wv_min(t2);
	for (int hi = n; hi > t2; hi -= 64) {   /* from the top, 64 entries a step: every lane has read before any writes */
		const int lo = hi - 64 > t2 ? hi - 64 : t2, k = lo + lane;
		const uint16_t val = k < hi ? v.ord[k] : (uint16_t)0;
		ssg_wave_memsync();
		if (k < hi) v.ord[k + 1] = val;
		ssg_wave_memsync();
	}
	SSG_LANE0(v.ord[t2] = (uint16_t)v.nrec; v.key[v.nrec] = kb);
	++v.n; ++v.nrec;
	return t2;
}

/* wv_sort_dedup_incr (k_sdp.h) on the view: the list is the output of an earlier re-sort with ONE new region at ord[xpos].  Returns the new length, or -1
 * (view untouched) when the outcome depends on the order of equal keys. */
SSG_DEVFN int mk_sort_dedup_incr(const ssg_mem_opt_t &opt, ssg_mk_view_t &v, int xpos)
{
	const int lane = wv_lane(), n = v.n;
	ssg_wave_memsync();
	const uint16_t xid = v.ord[xpos];
	const ssg_sdp_key_t x = v.key[xid];
	const int64_t gap = opt.max_chain_gap;
	const int64_t NONE_LO = INT64_MIN, NONE_HI = INT64_MAX;
	int tie = 0;
	int64_t ystar = NONE_LO, ycirc = NONE_HI;   /* case 1: largest re that drops x; case 2: smallest re that drops x */
	for (int i = lane; i < n; i += 64) {
		if (i == xpos) continue;
		const ssg_sdp_key_t y = v.key[v.ord[i]];
		const int64_t yre = y.re, yrb = y.rb; const int yqb = y.qb, yqe = y.qe, ysc = y.score;
		if (yre == x.re) tie = 1;
		if (ysc == x.score && yrb == x.rb && yqb == x.qb) tie = 1;
		if (y.rid != x.rid) continue;
		if (yre < x.re) { /* p = x, q = y */
			if (x.rb < yre + gap) {
				const int64_t or_ = yre - x.rb, oq = yqb < x.qb ? yqe - x.qb : x.qe - yqb;
				const int64_t mr = yre - yrb < x.re - x.rb ? yre - yrb : x.re - x.rb, mq = yqe - yqb < x.qe - x.qb ? yqe - yqb : x.qe - x.qb;
				if (or_ > opt.mask_level_redun * mr && oq > opt.mask_level_redun * mq && x.score < ysc) ystar = ystar > yre ? ystar : yre;
			}
		} else { /* p = y, q = x */
			if (yrb < x.re + gap) {
				const int64_t or_ = x.re - yrb, oq = x.qb < yqb ? x.qe - yqb : yqe - x.qb;
				const int64_t mr = x.re - x.rb < yre - yrb ? x.re - x.rb : yre - yrb, mq = x.qe - x.qb < yqe - yqb ? x.qe - x.qb : yqe - yqb;
				if (or_ > opt.mask_level_redun * mr && oq > opt.mask_level_redun * mq && !(ysc < x.score)) ycirc = ycirc < yre ? ycirc : yre;
			}
		}
	}
	if (wv_ballot(tie)) return -1;
	ystar = wv_max64(ystar); ycirc = -wv_max64(-ycirc);
	const bool x_dead1 = ystar != NONE_LO, x_dead = x_dead1 || ycirc != NONE_HI;
	/* second pass: who is dropped, and the new positions */
	int base = 0, bad = 0, x_rank = 0;
	for (int i0 = 0; i0 < n; i0 += 64) {
		const int i = i0 + lane;
		int alive = 0;
		uint16_t id = 0;
		ssg_sdp_key_t r; r.re = r.rb = 0; r.qb = r.qe = r.score = r.rid = 0;
		if (i < n && i != xpos) {
			id = v.ord[i]; r = v.key[id];
			alive = 1;
			if (r.rid == x.rid) {
				if (r.re < x.re) {
					if (x.rb < r.re + gap) {
						const int64_t or_ = r.re - x.rb, oq = r.qb < x.qb ? r.qe - x.qb : x.qe - r.qb;
						const int64_t mr = r.re - r.rb < x.re - x.rb ? r.re - r.rb : x.re - x.rb, mq = r.qe - r.qb < x.qe - x.qb ? r.qe - r.qb : x.qe - x.qb;
						if (or_ > opt.mask_level_redun * mr && oq > opt.mask_level_redun * mq && !(x.score < r.score)) {
							if (!x_dead1 || r.re > ystar) alive = 0;
							else if (r.re == ystar) bad = 1;
						}
					}
				} else if (!x_dead1) {
					if (r.rb < x.re + gap) {
						const int64_t or_ = x.re - r.rb, oq = x.qb < r.qb ? x.qe - r.qb : r.qe - x.qb;
						const int64_t mr = x.re - x.rb < r.re - r.rb ? x.re - x.rb : r.re - r.rb, mq = x.qe - x.qb < r.qe - r.qb ? x.qe - x.qb : r.qe - r.qb;
						if (or_ > opt.mask_level_redun * mr && oq > opt.mask_level_redun * mq && r.score < x.score) {
							if (ycirc == NONE_HI || r.re < ycirc) alive = 0;
							else if (r.re == ycirc) bad = 1;
						}
					}
				}
			}
		}
		/* survivors keep their (score, rb, qb) order; x (put behind all regions of >= score by mem_matesw) moves to its rank */
		const int before_x = alive && ((r.score > x.score) | ((r.score == x.score) & ((r.rb < x.rb) | ((r.rb == x.rb) & (r.qb < x.qb)))));
		const unsigned long long bal = wv_ballot(alive);
		if (alive) v.alt[base + wv_rank_of(bal) + (!x_dead && !before_x)] = id;
		base += __popcll(bal);
		x_rank += __popcll(wv_ballot(before_x));
	}
	if (wv_ballot(bad)) return -1;
	if (!x_dead) { SSG_LANE0(v.alt[x_rank] = xid); ++base; }
	ssg_wave_memsync();
	uint16_t *t = v.ord; v.ord = v.alt; v.alt = t;
	v.n = base;
	return base;
}

/* the key-based full sort of wv_sort_dedup_fast (k_sdp.h; no patching) on the view: the same sorts, the same tie replays of upstream's introsort starting
 * from the list order, the same scan; the result is the new order.  A list of at most one entry is returned as it is, as there. */
SSG_DEVFN int mk_sort_dedup_full(const ssg_mem_opt_t &opt, ssg_mk_view_t &v)
{
	const int n = v.n;
	if (n <= 1) return n;
	const int lane = wv_lane();
	ssg_sdp_key_t *const key = v.key; uint64_t *const skey = v.skey; uint16_t *const ord = v.ord, *const alt = v.alt;
	ssg_wave_memsync();
	for (int i = lane; i < n; i += 64) skey[i] = (uint64_t)key[ord[i]].re;
	ssg_wave_memsync();
	if (wv_rank_u64(skey, n, [&](int t, int rank, int ties) { if (ties == 1) alt[rank] = ord[t]; })) { /* ties in `re`: upstream's unstable sort decides */
		SSG_LANE0(for (int t = 0; t < n; ++t) alt[t] = ord[t]; ssg_key_re_lt lt = { key }; ssg_introsort(alt, (long)n, lt));
	}
	ssg_wave_memsync();
	for (int base = 0; base < n; base += 64) {   /* the redundancy scan: lane 0 runs upstream's step for the entries that have a near predecessor, in order */
		const int i = base + lane;
		bool near = false;
		if (i >= 1 && i < n) { const ssg_sdp_key_t &p = key[alt[i]], &q = key[alt[i-1]]; near = p.rid == q.rid && p.rb < q.re + opt.max_chain_gap; }
		unsigned long long todo = wv_ballot(near);
		if (todo) {
			if (lane == 0) {
				while (todo) {
					const int ii = base + (int)__builtin_ctzll(todo); todo &= todo - 1;
					ssg_sdp_key_t *p = &key[alt[ii]];
					for (int j = ii - 1; j >= 0 && p->rid == key[alt[j]].rid && p->rb < key[alt[j]].re + opt.max_chain_gap; --j) {
						ssg_sdp_key_t *q = &key[alt[j]];
						int64_t or_, oq, mr, mq;
						if (q->qe == q->qb) continue;
						or_ = q->re - p->rb;
						oq = q->qb < p->qb ? q->qe - p->qb : p->qe - q->qb;
						mr = q->re - q->rb < p->re - p->rb ? q->re - q->rb : p->re - p->rb;
						mq = q->qe - q->qb < p->qe - p->qb ? q->qe - q->qb : p->qe - p->qb;
						if (or_ > opt.mask_level_redun * mr && oq > opt.mask_level_redun * mq) {
							if (p->score < q->score) { p->qe = p->qb; break; }
							else q->qe = q->qb;
						}
					}
				}
			}
			ssg_wave_memsync();
		}
	}
	ssg_wave_memsync();
	int n2 = 0;   /* survivors, in order, back into ord[] */
	for (int base = 0; base < n; base += 64) {
		const int i = base + lane;
		const uint16_t id = i < n ? alt[i] : (uint16_t)0;
		const unsigned long long live = wv_ballot(i < n && key[id].qe > key[id].qb);
		if (i < n && (live >> lane & 1)) ord[n2 + wv_rank_of(live)] = id;
		n2 += __popcll(live);
	}
	ssg_wave_memsync();
	int wide = 0;   /* (score descending, rb, qb) as one 64-bit key when the fields fit */
	for (int t = lane; t < n2; t += 64) {
		const ssg_sdp_key_t &k = key[ord[t]];
		wide |= k.score < 0 || k.score > 0xfffe || k.rb < 0 || k.rb >= (int64_t)1 << 38 || k.qb < 0 || k.qb > 1023;
		skey[t] = (uint64_t)(0xffff - k.score) << 48 | (uint64_t)k.rb << 10 | (uint64_t)k.qb;
	}
	const bool packed = wv_ballot(wide) == 0;
	ssg_wave_memsync();
	if (packed ? wv_rank_u64(skey, n2, [&](int t, int rank, int ties) { if (ties == 1) alt[rank] = ord[t]; })
	           : wv_rank_sort(key, ord, alt, n2, ssg_sc_less())) { /* identical (score, rb, qb): tie order selects the survivor */
		SSG_LANE0(for (int t = 0; t < n2; ++t) alt[t] = ord[t]; ssg_key_sc_lt lt = { key }; ssg_introsort(alt, (long)n2, lt));
	}
	ssg_wave_memsync();
	/* identical hits: the later one of two neighbours goes */
	for (int i = 1 + lane; i < n2; i += 64) {
		const ssg_sdp_key_t &x = key[alt[i]], &y = key[alt[i-1]];
		if (x.score == y.score && x.rb == y.rb && x.qb == y.qb) key[alt[i]].qe = x.qb;
	}
	ssg_wave_memsync();
	int m = n2 < 1 ? n2 : 1;
	for (int base = 1; base < n2; base += 64) {
		const int i = base + lane;
		const uint16_t id = i < n2 ? alt[i] : (uint16_t)0;
		const unsigned long long live = wv_ballot(i < n2 && key[id].qe > key[id].qb);
		ssg_wave_memsync();   /* every lane has read its entry before any is overwritten */
		if (i < n2 && (live >> lane & 1)) alt[m + wv_rank_of(live)] = id;
		m += __popcll(live);
	}
	ssg_wave_memsync();
	v.ord = alt; v.alt = ord; v.n = m;
	return m;
}

/* what the replay of one side leaves to the end of the pair */
struct ssg_mk_side_t { int n, changed, ones; const uint16_t *ord; };

/* upstream mem_matesw for one anchor (rb, rid) against the view v of the mate's list, as wv_matesw (k_pair.h) does it on the records; jres: the anchor's four
 * slots.  Returns the windows tried, or -1 with *why set (nothing the pair's replay by ssg_k_matesw depends on has been written). */
SSG_DEVFN int mk_anchor(const ssg_index_view_t &ix, const ssg_mem_opt_t &opt, const ssg_pestat_t *pes, const int64_t arb, const int arid, const int l_ms,
                        ssg_alnreg_t *ma, const int ma_cap, ssg_mk_view_t &v, ssg_mk_big_t *B, int *fixed, ssg_mk_side_t *st, const ssg_msres_t *jres,
                        const int tcap, unsigned long long *cells, int *why)
{
	const int64_t l_pac = ix.l_pac;
	const int lane = wv_lane();
	int i, r, skip[4], n = 0, rid = -1;
	for (r = 0; r < 4; ++r) skip[r] = pes[r].failed ? 1 : 0;
	{
		int seen = 0;
		ssg_wave_memsync();
		for (i = lane; i < v.n; i += 64) {
			int64_t dist;
			r = ssg_infer_dir(l_pac, arb, v.key[v.ord[i]].rb, &dist);
			if (dist >= pes[r].low && dist <= pes[r].high) seen |= 1 << r;
		}
		for (r = 0; r < 4; ++r) if (wv_ballot(seen >> r & 1)) skip[r] = 1;
	}
	if (skip[0] + skip[1] + skip[2] + skip[3] == 4) return 0;
	for (r = 0; r < 4; ++r) {
		int is_rev, is_larger, xpos = -1;
		int64_t rb, re;
		if (skip[r]) continue;
		is_rev = (r >> 1 != (r & 1));
		is_larger = !(r >> 1);
		if (!is_rev) {
			rb = is_larger ? arb + pes[r].low : arb - pes[r].high;
			re = (is_larger ? arb + pes[r].high : arb - pes[r].low) + l_ms;
		} else {
			rb = (is_larger ? arb + pes[r].low : arb - pes[r].high) - l_ms;
			re = is_larger ? arb + pes[r].high : arb - pes[r].low;
		}
		if (rb < 0) rb = 0;
		if (re > l_pac << 1) re = l_pac << 1;
		if (rb < re) { /* upstream bns_fetch_seq around the window's midpoint */
			int rv; rid = ssg_pos2rid(ix, ssg_depos(ix, (rb + re) >> 1, &rv));
			int64_t far_beg = ix.ctg_off[rid], far_end = far_beg + ix.ctg_len[rid];
			if (rv) { int64_t t2 = far_beg; far_beg = (l_pac << 1) - far_end; far_end = (l_pac << 1) - t2; }
			rb = rb > far_beg ? rb : far_beg;
			re = re < far_end ? re : far_end;
		}
		if (arid == rid && re - rb >= opt.min_seed_len) {
			if (re - rb > tcap) { *why = SSG_MK_WHY_ERR; return -1; }   /* ssg_k_matesw's error 1 */
			const int xtra = SSG_KSW_XSUBO | SSG_KSW_XSTART | (l_ms * opt.a < 250 ? SSG_KSW_XBYTE : 0) | (opt.min_seed_len * opt.a);
			const ssg_msres_t s = jres[r];
			const int pre = wv_get(s.state >= 1 && s.rb == rb && s.tlen == (int)(re - rb) ? s.state : 0, 0);
			if (!pre) { *why = SSG_MK_WHY_SLOT; return -1; }
			const int score = wv_get(s.score, 0), te = wv_get(s.te, 0), qe = wv_get(s.qe, 0);
			if (pre == 1 && ssg_align2_has_rev(xtra, score)) { *why = SSG_MK_WHY_REV; return -1; }
			const int tb = pre == 2 ? wv_get(s.tb, 0) : -1, qb = pre == 2 ? wv_get(s.qb, 0) : -1;
			*cells += (unsigned long long)(re - rb) * l_ms;
			if (score >= opt.min_seed_len && qb >= 0) {
				if (v.n >= ma_cap || v.nrec >= ma_cap) { *why = SSG_MK_WHY_ROOM; return -1; }   /* (v.n >= ma_cap is ssg_k_matesw's error 2) */
				if (v.nrec >= SSG_MK_BIGCAP) { *why = SSG_MK_WHY_BIG; return -1; }
				if (!v.big && v.nrec >= SSG_SDP_CAP) mk_to_big(v, B);
				ssg_alnreg_t b;
				b.rb = b.re = 0; b.qb = b.qe = 0; b.truesc = b.sub = b.alt_sc = b.sub_n = b.w = b.secondary_all = b.seedlen0 = b.n_comp = 0; b.frac_rep = 0; b.hash = 0;
				b.rid = arid;
				b.qb = is_rev ? l_ms - (qe + 1) : qb;
				b.qe = is_rev ? l_ms - qb : qe + 1;
				b.rb = is_rev ? (l_pac << 1) - (rb + te + 1) : rb + tb;
				b.re = is_rev ? (l_pac << 1) - (rb + tb) : rb + te + 1;
				b.score = score;
				b.csub = wv_get(s.score2, 0);
				b.secondary = -1;
				b.seedcov = (int)((b.re - b.rb < b.qe - b.qb ? b.re - b.rb : b.qe - b.qb) >> 1);
				SSG_LANE0(ma[v.nrec] = b);   /* head-room: past n_reg until the pair is decided */
				ssg_sdp_key_t kb; kb.re = b.re; kb.rb = b.rb; kb.qb = b.qb; kb.qe = b.qe; kb.score = b.score; kb.rid = b.rid;
				xpos = mk_insert(v, kb);
				st->changed = 1;
			}
			++n;
		}
		if (n) { /* upstream re-sorts after every attempted window once one was tried */
			if (*fixed) {
				if (xpos >= 0) {
					if (mk_sort_dedup_incr(opt, v, xpos) < 0) { *why = SSG_MK_WHY_TIE; return -1; }
					st->changed = st->ones = 1;
				}
			} else if (v.n > 1) { (void)mk_sort_dedup_full(opt, v); st->changed = st->ones = 1; }
			*fixed = 1;
		}
	}
	return n;
}

/* the records of a decided list, gathered once by position through the wave's buffer: a[k] = a[ord[k]], k < m */
SSG_DEVFN void mk_store(ssg_alnreg_t *a, const uint16_t *ord, int m, ssg_alnreg_t *tmp, int ones)
{
	static_assert(sizeof(ssg_alnreg_t) % 8 == 0, "ssg_alnreg_t is copied in 8-byte words");
	constexpr int W = (int)(sizeof(ssg_alnreg_t) / 8);
	const int lane = wv_lane();
	uint64_t *const tw = (uint64_t*)tmp; uint64_t *const aw = (uint64_t*)a;
	ssg_wave_memsync();
	for (int t = lane; t < m * W; t += 64) { const int k = t / W, w = t - k * W; tw[t] = ((const uint64_t*)&a[ord[k]])[w]; }
	ssg_wave_memsync();
	if (ones) for (int k = lane; k < m; k += 64) tmp[k].n_comp = 1;
	ssg_wave_memsync();
	for (int t = lane; t < m * W; t += 64) aw[t] = tw[t];
	ssg_wave_memsync();
}

/*
 * One wavefront per listed pair, from a heaviest-first queue.  todo[0 .. *n_todo): the pairs; jbase[2 kq + i]: first slot of side i of the kq-th of them.
 * gtmp: SSG_MK_BIGCAP records per wave; slab: one ssg_mk_big_t per wave.  Pairs given up: left[], with their slot bases in lbase[] (the layout of jbase),
 * counted in cnt[0]; cnt: SSG_MK_NCNT counters.  cells / n_rescue as in ssg_k_matesw ([0] windows, [1] windows taken from slots: all of them here).
 */
__global__ void __launch_bounds__(64 * SSG_MK_WAVES) ssg_k_matesw_keys(ssg_index_view_t ix, ssg_mem_opt_t opt, const int64_t *read_off, const int64_t *reg_off, ssg_alnreg_t *regs,
                                  int32_t *n_reg, const int32_t *pair_batch, const ssg_pestat_t *pes_all, ssg_alnreg_t *gtmp, ssg_mk_big_t *slab,
                                  unsigned long long *cells, unsigned long long *n_rescue, const int32_t *todo, const unsigned int *n_todo, unsigned int *queue,
                                  const ssg_msres_t *jres, const int64_t *jbase, const uint8_t *sdp_fixed, int tcap,
                                  int32_t *left, int64_t *lbase, unsigned int *cnt)
{
	__shared__ ssg_mk_lds_t lds[SSG_MK_WAVES];
	const int wslot = (int)(threadIdx.x >> 6), lane = wv_lane();
	const long wave0 = (long)blockIdx.x * (blockDim.x >> 6) + wslot;
	ssg_mk_lds_t *const L = &lds[wslot];
	ssg_mk_big_t *const B = slab + wave0;
	ssg_alnreg_t *const tmp = gtmp + wave0 * (long)SSG_MK_BIGCAP;
	unsigned long long nc = 0, nres = 0;
	unsigned int ntaken = 0;
	const long n_work = (long)*n_todo;
	for (;;) {
		const long kq = wv_queue_pop(queue);
		if (kq >= n_work) break;
		const long p = todo[kq];
		const ssg_pestat_t *pes = pes_all + (long)pair_batch[p] * 4;
		ssg_alnreg_t *a[2] = { regs + reg_off[2*p], regs + reg_off[2*p+1] };
		const int an[2] = { n_reg[2*p], n_reg[2*p+1] };
		const int cap[2] = { (int)(reg_off[2*p+1] - reg_off[2*p]), (int)(reg_off[2*p+2] - reg_off[2*p+1]) };
		int why = 0, nb[2] = {0, 0};
		unsigned long long pc = 0, pres = 0;
		ssg_mk_side_t st[2] = { { an[0], 0, 0, 0 }, { an[1], 0, 0, 0 } };   /* st[t]: the list of read t */
		if (an[0] > SSG_SDP_BIG || an[1] > SSG_SDP_BIG || an[0] > cap[0] || an[1] > cap[1]) why = SSG_MK_WHY_BIG;
		for (int i = 0; i < 2 && !why; ++i) { /* b[i] = hits within pen_unpaired of the best, taken BEFORE any rescue (upstream order) */
			int c = 0;
			const int thr = an[i] ? a[i][0].score - opt.pen_unpaired : 0;
			for (int j = lane; j < an[i]; j += 64) if (a[i][j].score >= thr) ++c;
			c = wv_sum(c);
			nb[i] = c < opt.max_matesw ? c : opt.max_matesw;
			if (nb[i] > SSG_MK_ANCH) why = SSG_MK_WHY_ERR;   /* ssg_k_matesw's error 3 */
		}
		if (!why && nb[0] + nb[1] > 0) {
			ssg_wave_memsync();
			for (int i = 0; i < 2; ++i) { /* the first nb[i] qualifying hits, in list order: what mem_matesw reads of them */
				const int thr = an[i] ? a[i][0].score - opt.pen_unpaired : 0;
				int c2 = 0;
				for (int j0 = 0; j0 < an[i] && c2 < nb[i]; j0 += 64) {
					const int j2 = j0 + lane;
					const int f = j2 < an[i] && a[i][j2].score >= thr;
					const unsigned long long bal = wv_ballot(f);
					const int at = c2 + wv_rank_of(bal);
					if (f && at < nb[i]) { L->arb[i][at] = a[i][j2].rb; L->arid[i][at] = a[i][j2].rid; }
					c2 += __popcll(bal);
				}
			}
			ssg_wave_memsync();
			for (int i = 0; i < 2 && !why; ++i) {
				if (nb[i] == 0) continue;
				const int t = !i;
				const int l_ms = (int)(read_off[2*p + t + 1] - read_off[2*p + t]);
				int fixed = (int)sdp_fixed[2*p + t];
				ssg_mk_view_t v;
				mk_load(v, L, B, a[t], an[t]);
				for (int j = 0; j < nb[i] && !why; ++j) {
					const int64_t arb = L->arb[i][j]; const int arid = L->arid[i][j];
					const int w = mk_anchor(ix, opt, pes, arb, arid, l_ms, a[t], cap[t], v, B, &fixed, &st[t], jres + jbase[2*kq + i] + 4 * j, tcap, &pc, &why);
					if (w > 0) pres += (unsigned long long)w;
				}
				if (why) break;
				st[t].n = v.n;
				if (st[t].changed) {
					if (i == 0) { /* the first side's order waits for the second side's verdict */
						uint16_t *keep = v.big ? B->keep : L->keep;
						ssg_wave_memsync();
						for (int k = lane; k < v.n; k += 64) keep[k] = v.ord[k];
						ssg_wave_memsync();
						st[t].ord = keep;
					} else st[t].ord = v.ord;
				}
			}
			if (!why)
				for (int t = 0; t < 2; ++t) if (st[t].changed) {
					mk_store(a[t], st[t].ord, st[t].n, tmp, st[t].ones);
					if (lane == 0) n_reg[2*p + t] = st[t].n;
				}
		}
		if (why) {
			if (lane == 0) {
				const unsigned int k = atomicAdd(&cnt[0], 1u);
				left[k] = (int32_t)p; lbase[2 * (long)k] = jbase[2*kq]; lbase[2 * (long)k + 1] = jbase[2*kq + 1];
				atomicAdd(&cnt[1 + why], 1u);
			}
		} else { nc += pc; nres += pres; ++ntaken; }
	}
	if (lane == 0) {
		if (nc) atomicAdd(cells, nc);
		if (nres) { atomicAdd(n_rescue, nres); atomicAdd(n_rescue + 1, nres); }
		if (ntaken) atomicAdd(&cnt[1], ntaken);
		if (nres) atomicAdd(&cnt[1 + SSG_MK_NWHY], (unsigned int)nres);
	}
}
#endif
