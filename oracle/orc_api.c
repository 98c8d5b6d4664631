/*
 * oracle/orc_api.c -- CPU ORACLE (test infrastructure): flat, ctypes-friendly wrappers used by
 * tests/ to compare the HIP path with the oracle stage by stage.
 */
#include <stdlib.h>
#include <string.h>
#include "orc.h"

typedef struct {
	int64_t rb, re;
	int32_t qb, qe, rid, score, truesc, sub, alt_sc, csub, sub_n, w, seedcov, secondary, secondary_all, seedlen0, n_comp;
	float frac_rep;
	uint64_t hash;
} orc_flatreg_t;

static void flatten(const orc_alnreg_t *a, orc_flatreg_t *f)
{
	f->rb = a->rb; f->re = a->re; f->qb = a->qb; f->qe = a->qe; f->rid = a->rid; f->score = a->score; f->truesc = a->truesc;
	f->sub = a->sub; f->alt_sc = a->alt_sc; f->csub = a->csub; f->sub_n = a->sub_n; f->w = a->w; f->seedcov = a->seedcov;
	f->secondary = a->secondary; f->secondary_all = a->secondary_all; f->seedlen0 = a->seedlen0; f->n_comp = a->n_comp;
	f->frac_rep = a->frac_rep; f->hash = a->hash;
}

static void unflatten(const orc_flatreg_t *f, orc_alnreg_t *a)
{
	memset(a, 0, sizeof(*a));
	a->rb = f->rb; a->re = f->re; a->qb = f->qb; a->qe = f->qe; a->rid = f->rid; a->score = f->score; a->truesc = f->truesc;
	a->sub = f->sub; a->alt_sc = f->alt_sc; a->csub = f->csub; a->sub_n = f->sub_n; a->w = f->w; a->seedcov = f->seedcov;
	a->secondary = f->secondary; a->secondary_all = f->secondary_all; a->seedlen0 = f->seedlen0; a->n_comp = f->n_comp;
	a->frac_rep = f->frac_rep; a->hash = f->hash;
}
static orc_alnreg_v list_of(const orc_flatreg_t *f, int64_t n)
{
	orc_alnreg_v v = { (size_t)n, (size_t)n, malloc(sizeof(orc_alnreg_t) * (size_t)(n + 1)) };
	for (int64_t k = 0; k < n; ++k) unflatten(&f[k], &v.a[k]);
	return v;
}

orc_opt_t *orc_api_opt_new(void) { orc_opt_t *o = malloc(sizeof(orc_opt_t)); orc_opt_init(o); return o; }
/* scoring of the stage-level checks (bwa mem -A -B -O -E): a, b, gap open / extend for deletions and insertions */
void orc_api_opt_scores(orc_opt_t *o, int a, int b, int o_del, int e_del, int o_ins, int e_ins)
{ o->a = a; o->b = b; o->o_del = o_del; o->e_del = e_del; o->o_ins = o_ins; o->e_ins = e_ins; orc_fill_scmat(o); }
/* the chain filter's knobs (bwa mem -D, -W, -N and the compiled-in mask_level / max_chain_gap), for the chaining kernels' tests */
void orc_api_opt_chain(orc_opt_t *o, float drop_ratio, float mask_level, int min_chain_weight, int max_chain_extend, int max_chain_gap)
{ o->drop_ratio = drop_ratio; o->mask_level = mask_level; o->min_chain_weight = min_chain_weight; o->max_chain_extend = max_chain_extend; o->max_chain_gap = max_chain_gap; }
/* the seeding stage's knobs (bwa mem -k, -r, -c, -y and the compiled-in split_width), for the seeding reference's tests */
void orc_api_opt_seed(orc_opt_t *o, int min_seed_len, float split_factor, int split_width, int max_occ, int64_t max_mem_intv)
{ o->min_seed_len = min_seed_len; o->split_factor = split_factor; o->split_width = split_width; o->max_occ = max_occ; o->max_mem_intv = (uint64_t)max_mem_intv; }
/* the paired-end decision stage's knobs (bwa mem -M / -P through flag, -T, -U, -h and the compiled-in mapQ coefficients), for the pairing reference's tests */
void orc_api_opt_pair(orc_opt_t *o, int flag, int max_XA_hits, float mapQ_coef_len, int mapQ_coef_fac, int T, int pen_unpaired)
{ o->flag = flag; o->max_XA_hits = max_XA_hits; o->mapQ_coef_len = mapQ_coef_len; o->mapQ_coef_fac = mapQ_coef_fac; o->T = T; o->pen_unpaired = pen_unpaired; }
/* the chaining stage's remaining knobs (bwa mem -w, -k, -c), for the chaining reference's tests */
void orc_api_opt_chain2(orc_opt_t *o, int w, int min_seed_len, int max_occ) { o->w = w; o->min_seed_len = min_seed_len; o->max_occ = max_occ; }
/* the region stage's knobs (bwa mem -w, -d, -L and the compiled-in max_chain_gap / mask_level_redun), for the region reference's tests */
void orc_api_opt_regions(orc_opt_t *o, int w, int zdrop, int pen_clip5, int pen_clip3, int max_chain_gap, float mask_level_redun)
{ o->w = w; o->zdrop = zdrop; o->pen_clip5 = pen_clip5; o->pen_clip3 = pen_clip3; o->max_chain_gap = max_chain_gap; o->mask_level_redun = mask_level_redun; }
void orc_api_free(void *p) { free(p); }

/* The chaining stage on seeds and intervals given by the caller (tests/test_chain_reference.py; the library's twin is ssg_dbg_chain): read r's seeds are
 * seeds[4 * seed_off[r] .. 4 * seed_off[r + 1]) as (rbeg, qbeg, len, rid) in visiting order, its intervals intv[intv_off[r] .. intv_off[r + 1]).  Out, per read
 * (chain_off[n_reads + 1]): the chains as orc_mem_chain_flt leaves them AFTER ITS SORT, those it marks kept = 0 included -- 7 values a chain: pos, rid, n, w, kept,
 * the bits of frac_rep, where its n seed indices (counted from the read's first seed, insertion order) begin in chain_seeds.  Room for one chain and one index per
 * seed suffices.  The container of mem_chain is the calling thread's (orc_api_set_chain_container). */
void orc_api_chain(const orc_opt_t *opt, int64_t l_pac, int n_reads, const int32_t *read_len, const int64_t *seed_off, const int64_t *seeds,
                   const int64_t *intv_off, const orc_intv_t *intv, int64_t *chain_off, int64_t *chains, int32_t *chain_seeds)
{
	int64_t nc = 0, nq = 0;
	for (int r = 0; r < n_reads; ++r) {
		const int64_t s0 = seed_off[r], ns = seed_off[r + 1] - s0;
		orc_seed_t *sd = calloc((size_t)(ns + 1), sizeof(orc_seed_t)); int *rd = malloc(sizeof(int) * (size_t)(ns + 1));
		for (int64_t k = 0; k < ns; ++k) {   /* (score carries the seed's index through the chain lists: nothing in this stage reads it) */
			const int64_t *p = seeds + 4 * (s0 + k);
			sd[k].rbeg = p[0]; sd[k].qbeg = (int32_t)p[1]; sd[k].len = (int32_t)p[2]; sd[k].score = (int32_t)k; rd[k] = (int)p[3];
		}
		orc_chain_v c = orc_chain_seeds(opt, l_pac, ns, sd, rd);
		const float frac_rep = orc_frac_rep(opt, read_len[r], (int)(intv_off[r + 1] - intv_off[r]), intv + intv_off[r]);
		for (size_t i = 0; i < c.n; ++i) c.a[i].frac_rep = frac_rep;
		const int n = orc_mem_chain_flt_mark(opt, (int)c.n, c.a);
		chain_off[r] = nc;
		for (int i = 0; i < n; ++i) {
			const orc_chain_t *x = &c.a[i];
			int64_t *o = chains + 7 * nc++;
			uint32_t fb; memcpy(&fb, &x->frac_rep, 4);
			o[0] = x->pos; o[1] = x->rid; o[2] = x->n; o[3] = x->w; o[4] = x->kept; o[5] = fb; o[6] = nq;
			for (int j = 0; j < x->n; ++j) chain_seeds[nq++] = x->seeds[j].score;
			free(x->seeds);
		}
		free(c.a); free(sd); free(rd);
	}
	chain_off[n_reads] = nc;
}

/* the paired-end decision stage on region lists given by the caller (tests/test_pair_reference.py; the library's twins are ssg_dbg_pestat / ssg_dbg_pair_final):
 * read r's regions are regs[reg_off[r] .. reg_off[r + 1]), read 1 and read 2 of a pair interleaved.
 * orc_api_pestat: orc_mem_pestat over the pairs of each batch, n_batches x 4 models. */
void orc_api_pestat(const orc_opt_t *opt, const orc_idx_t *idx, int n_pairs, const int64_t *reg_off, const orc_flatreg_t *regs, const int32_t *pair_batch, int n_batches, orc_pestat_t *pes)
{
	orc_alnreg_v *v = malloc(sizeof(orc_alnreg_v) * (size_t)(2 * n_pairs + 1));
	for (int b = 0; b < n_batches; ++b) {
		int n = 0;
		for (int p = 0; p < n_pairs; ++p) if (pair_batch[p] == b) for (int i = 0; i < 2; ++i) v[n++] = list_of(regs + reg_off[2 * p + i], reg_off[2 * p + i + 1] - reg_off[2 * p + i]);
		orc_mem_pestat(opt, idx->bns->l_pac, n, v, &pes[4 * b]);
		for (int k = 0; k < n; ++k) free(v[k].a);
	}
	free(v);
}
/* orc_api_pair_final: orc_mem_mark_primary_se, orc_mem_pair and the decision of orc_mem_sam_pe (orc_mem_pe_records) for every pair, pair p with id id0 + p:
 * regs_out the lists as the stage leaves them, req_off[2 n_pairs + 1] and req (room for 2 * regions + reads entries) the records, reg counted from regs[0]. */
void orc_api_pair_final(const orc_opt_t *opt, const orc_idx_t *idx, int n_pairs, int64_t id0, const int64_t *reg_off, const orc_flatreg_t *regs, const orc_pestat_t pes[4],
                        orc_flatreg_t *regs_out, int64_t *req_off, orc_pe_rec_t *req)
{
	int64_t nreq = 0;
	for (int p = 0; p < n_pairs; ++p) {
		orc_alnreg_v a[2]; orc_pe_rec_t *rec[2]; int n_rec[2];
		for (int i = 0; i < 2; ++i) { a[i] = list_of(regs + reg_off[2 * p + i], reg_off[2 * p + i + 1] - reg_off[2 * p + i]); rec[i] = malloc(sizeof(orc_pe_rec_t) * (2 * a[i].n + 1)); }
		orc_mem_pe_records(opt, idx, pes, (uint64_t)(id0 + p), a, rec, n_rec);
		for (int i = 0; i < 2; ++i) {
			req_off[2 * p + i] = nreq;
			for (int k = 0; k < n_rec[i]; ++k) { req[nreq] = rec[i][k]; if (req[nreq].reg >= 0) req[nreq].reg += (int32_t)reg_off[2 * p + i]; ++nreq; }
			for (size_t k = 0; k < a[i].n; ++k) flatten(&a[i].a[k], &regs_out[reg_off[2 * p + i] + k]);
			free(a[i].a); free(rec[i]);
		}
	}
	req_off[2 * n_pairs] = nreq;
}

/* mem_collect_intv for one read; returns the number of intervals (out may be smaller than needed) */
int orc_api_collect_intv(const orc_opt_t *opt, const orc_idx_t *idx, int len, const uint8_t *seq, orc_intv_t *out, int cap)
{
	orc_intv_v mem = {0,0,0};
	orc_collect_intv(opt, idx->bwt, len, seq, &mem);
	int n = (int)mem.n;
	memcpy(out, mem.a, sizeof(orc_intv_t) * (n < cap ? n : cap));
	free(mem.a);
	return n;
}

/* the seeds mem_chain() visits for one read, in its order, before chaining (upstream bwamem.c mem_chain: for every interval of mem_collect_intv,
 * step = x[2] > max_occ ? x[2] / max_occ : 1, occurrences k = 0, step, ... while count < max_occ; rbeg = bwt_sa(x[0] + k); rid = bns_intv2rid,
 * seeds with rid < 0 are dropped by upstream and reported here with their rid).  out: 4 values per seed (rbeg, qbeg, len, rid).  Returns the count. */
int64_t orc_api_seeds(const orc_opt_t *opt, const orc_idx_t *idx, int len, const uint8_t *seq, int64_t *out, int64_t cap)
{
	orc_intv_v mem = {0,0,0};
	int64_t n = 0;
	if (len < opt->min_seed_len) return 0;
	orc_collect_intv(opt, idx->bwt, len, seq, &mem);
	for (size_t i = 0; i < mem.n; ++i) {
		const orc_intv_t *p = &mem.a[i];
		const int slen = (int)((uint32_t)p->info - (uint32_t)(p->info >> 32));
		const int64_t step = p->x[2] > (uint64_t)opt->max_occ ? (int64_t)(p->x[2] / opt->max_occ) : 1;
		int count = 0;
		for (int64_t k = 0; k < (int64_t)p->x[2] && count < opt->max_occ; k += step, ++count, ++n) {
			if (n >= cap) continue;
			const int64_t rbeg = (int64_t)orc_bwt_sa(idx->bwt, p->x[0] + k);
			out[4 * n] = rbeg; out[4 * n + 1] = (int64_t)(p->info >> 32); out[4 * n + 2] = slen; out[4 * n + 3] = orc_bns_intv2rid(idx->bns, rbeg, rbeg + slen);
		}
	}
	free(mem.a);
	return n;
}

/* mem_align1_core for a batch of reads; regs are appended to out (cap entries); reg_off[n+1] */
int64_t orc_api_align1_batch(const orc_opt_t *opt, const orc_idx_t *idx, int n_reads, const uint8_t *seq, const int64_t *off,
                             int64_t *reg_off, orc_flatreg_t *out, int64_t cap)
{
	int64_t tot = 0;
	for (int r = 0; r < n_reads; ++r) {
		int len = (int)(off[r+1] - off[r]);
		uint8_t *s = malloc(len + 1); memcpy(s, seq + off[r], len);
		orc_alnreg_v v = orc_mem_align1_core(opt, idx, len, s);
		reg_off[r] = tot;
		for (size_t i = 0; i < v.n; ++i) { if (tot < cap) flatten(&v.a[i], &out[tot]); ++tot; }
		free(v.a); free(s);
	}
	reg_off[n_reads] = tot;
	return tot;
}

/* The region stage on chains given by the caller (tests/test_region_reference.py; the library's twin is ssg_dbg_regions): orc_mem_chain2aln for every chain of a read
 * in order, then orc_mem_sort_dedup_patch, no change of behaviour.  The index is the 2-bit reference with its contig table.  Read r's seeds are
 * seeds[4 * seed_off[r] ..) as (rbeg, qbeg, len, unused) with score = len, its chains chains[3 * chain_off[r] ..) as (rid, n, the bits of frac_rep) with their seed
 * indices (counted from the read's first seed) one after another in chain_seeds.  Out: reg_off[n_reads + 1], out (cap entries; the count is returned), and
 * n_before[r] (may be NULL) = regions of read r before mem_sort_dedup_patch. */
int64_t orc_api_regions(const orc_opt_t *opt, const uint8_t *pac, int64_t l_pac, int n_ctg, const int64_t *ctg_off, const int32_t *ctg_len, int n_reads, const uint8_t *seq,
                        const int64_t *off, const int64_t *seed_off, const int64_t *seeds, const int64_t *chain_off, const int64_t *chains, const int32_t *chain_seeds,
                        int64_t *reg_off, orc_flatreg_t *out, int64_t cap, int32_t *n_before)
{
	orc_bns_t bns; orc_idx_t idx;
	memset(&bns, 0, sizeof(bns)); memset(&idx, 0, sizeof(idx));
	bns.l_pac = l_pac; bns.n_seqs = n_ctg; bns.anns = calloc((size_t)n_ctg, sizeof(orc_ann_t));
	for (int c = 0; c < n_ctg; ++c) { bns.anns[c].offset = ctg_off[c]; bns.anns[c].len = ctg_len[c]; }
	idx.bns = &bns; idx.pac = (uint8_t*)pac;
	int64_t tot = 0, q = 0;
	for (int r = 0; r < n_reads; ++r) {
		const int len = (int)(off[r + 1] - off[r]);
		uint8_t *s = malloc((size_t)len + 1); memcpy(s, seq + off[r], (size_t)len);
		orc_alnreg_v v = {0, 0, 0};
		for (int64_t k = chain_off[r]; k < chain_off[r + 1]; ++k) {
			orc_chain_t c; memset(&c, 0, sizeof(c));
			uint32_t fb = (uint32_t)chains[3 * k + 2];
			c.rid = (int)chains[3 * k]; c.n = c.m = (int)chains[3 * k + 1]; memcpy(&c.frac_rep, &fb, 4);
			c.seeds = malloc(sizeof(orc_seed_t) * (size_t)(c.n + 1));
			for (int j = 0; j < c.n; ++j) {
				const int64_t *p = seeds + 4 * (seed_off[r] + chain_seeds[q++]);
				c.seeds[j].rbeg = p[0]; c.seeds[j].qbeg = (int32_t)p[1]; c.seeds[j].len = c.seeds[j].score = (int32_t)p[2];
			}
			c.pos = c.seeds[0].rbeg;
			orc_mem_chain2aln(opt, &idx, len, s, &c, &v);
			free(c.seeds);
		}
		if (n_before) n_before[r] = (int32_t)v.n;
		v.n = (size_t)orc_mem_sort_dedup_patch(opt, &idx, s, (int)v.n, v.a);
		reg_off[r] = tot;
		for (size_t i = 0; i < v.n; ++i) { if (tot < cap) flatten(&v.a[i], &out[tot]); ++tot; }
		free(v.a); free(s);
	}
	reg_off[n_reads] = tot;
	free(bns.anns);
	return tot;
}

/* The record stage on regions and requests given by the caller (tests/test_record_reference.py; the library's twin is ssg_dbg_reg2aln): orc_mem_reg2aln for every
 * request, no change of behaviour.  req: 8 int32 a request (read, reg, kind, owner, flag, mapq, 0, 0: the library's ssg_alnreq_t; reg < 0: the unmapped record).
 * out: records in the library's ssg_aln_t layout, zeroed first; POS, rid, strand, CIGAR, NM, MD, score and sub are upstream's, flag = the request's | 0x100 for a
 * secondary region, mapq = the request's (mem_reg2sam overwrites mem_reg2aln's), reg_idx = owner, _pad = kind.  Upstream's record has no capacity: a CIGAR of more
 * than 64 operations or an MD of more than 319 characters is cut to the layout and counted in the return value; over[k] (may be NULL) = 1 for such a record.
 * The caller validates as ssg_dbg_reg2aln does: orc_mem_reg2aln trusts its region. */
typedef struct { int64_t pos; int32_t rid, flag, mapq, NM, score, sub, n_cigar, is_rev, l_md, reg_idx, xa_cnt, _pad; uint32_t cigar[64]; char md[320]; } orc_flataln_t;
int64_t orc_api_reg2aln(const orc_opt_t *opt, const uint8_t *pac, int64_t l_pac, int n_ctg, const int64_t *ctg_off, const int32_t *ctg_len, int n_reads, const uint8_t *seq,
                        const int64_t *off, int64_t n_regs, const orc_flatreg_t *regs, int64_t n_req, const int32_t *req, orc_flataln_t *out, uint8_t *over)
{
	orc_bns_t bns; orc_idx_t idx;
	int64_t n_over = 0;
	memset(&bns, 0, sizeof(bns)); memset(&idx, 0, sizeof(idx));
	bns.l_pac = l_pac; bns.n_seqs = n_ctg; bns.anns = calloc((size_t)n_ctg, sizeof(orc_ann_t));
	for (int c = 0; c < n_ctg; ++c) { bns.anns[c].offset = ctg_off[c]; bns.anns[c].len = ctg_len[c]; }
	idx.bns = &bns; idx.pac = (uint8_t*)pac;
	for (int64_t k = 0; k < n_req; ++k) {
		const int32_t *q = req + 8 * k;
		orc_flataln_t *o = &out[k];
		memset(o, 0, sizeof(*o));
		if (over) over[k] = 0;
		if (q[1] < 0) { o->pos = -1; o->rid = -1; o->flag = q[4] | 0x4; o->reg_idx = -1; continue; }
		orc_alnreg_t ar;
		unflatten(&regs[q[1]], &ar);
		const int len = (int)(off[q[0] + 1] - off[q[0]]);
		orc_aln_t a = orc_mem_reg2aln(opt, &idx, len, seq + off[q[0]], &ar);
		const char *md = (const char*)(a.cigar + a.n_cigar);
		const int l_md = (int)strlen(md);
		o->pos = a.pos; o->rid = a.rid; o->flag = q[4] | (a.flag & 0x100); o->mapq = q[5]; o->NM = (int32_t)a.NM; o->score = a.score; o->sub = a.sub;
		o->n_cigar = a.n_cigar; o->is_rev = a.is_rev; o->l_md = l_md; o->reg_idx = q[3]; o->xa_cnt = 0; o->_pad = q[2];
		memcpy(o->cigar, a.cigar, 4 * (size_t)(a.n_cigar < 64 ? a.n_cigar : 64));
		memcpy(o->md, md, (size_t)(l_md < 319 ? l_md : 319));
		if (a.n_cigar > 64 || l_md > 319) { ++n_over; if (over) over[k] = 1; }
		free(a.cigar);
	}
	free(bns.anns);
	return n_over;
}

/* ksw_global2 with the CIGAR copied out */
int orc_api_global2(const orc_opt_t *opt, int qlen, const uint8_t *q, int tlen, const uint8_t *t, int w, int *n_cigar, uint32_t *cigar, int cap)
{
	uint32_t *cg = 0; int n = 0;
	int sc = orc_ksw_global2(qlen, q, tlen, t, 5, opt->mat, opt->o_del, opt->e_del, opt->o_ins, opt->e_ins, w, &n, &cg);
	*n_cigar = n;
	memcpy(cigar, cg, 4 * (n < cap ? n : cap));
	free(cg);
	return sc;
}

void orc_api_extend2(const orc_opt_t *opt, int qlen, const uint8_t *q, int tlen, const uint8_t *t, int w, int end_bonus, int zdrop, int h0, int out[6])
{
	out[0] = orc_ksw_extend2(qlen, q, tlen, t, 5, opt->mat, opt->o_del, opt->e_del, opt->o_ins, opt->e_ins, w, end_bonus, zdrop, h0,
	                         &out[1], &out[2], &out[3], &out[4], &out[5]);
}

void orc_api_align2(const orc_opt_t *opt, int qlen, const uint8_t *q, int tlen, const uint8_t *t, int xtra, int out[7])
{
	uint8_t *qc = malloc(qlen + 1), *tc = malloc(tlen + 1);
	memcpy(qc, q, qlen); memcpy(tc, t, tlen);
	orc_kswr_t r = orc_ksw_align2(qlen, qc, tlen, tc, 5, opt->mat, opt->o_del, opt->e_del, opt->o_ins, opt->e_ins, xtra);
	out[0] = r.score; out[1] = r.te; out[2] = r.qe; out[3] = r.score2; out[4] = r.te2; out[5] = r.tb; out[6] = r.qb;
	free(qc); free(tc);
}

/* mem_process_seqs (PE) for one upstream batch; returns a malloc'd buffer with the SAM lines of all
 * reads in input order and fills sam_off[2*n_pairs+1]; pes_out receives the 4 insert-size models */
char *orc_api_process_pairs(const orc_opt_t *opt, const orc_idx_t *idx, int n_pairs, const uint8_t *seq, const int64_t *off,
                            const char **names, const char **quals, int64_t n_processed, const char *rg_id, int n_threads,
                            const orc_pestat_t *pes0, orc_pestat_t *pes_out, int64_t *sam_off)
{
	int n = 2 * n_pairs;
	orc_read_t *s = calloc(n, sizeof(orc_read_t));
	for (int i = 0; i < n; ++i) {
		s[i].l_seq = (int)(off[i+1] - off[i]);
		s[i].seq = malloc(s[i].l_seq + 1); memcpy(s[i].seq, seq + off[i], s[i].l_seq);
		s[i].name = (char*)names[i]; s[i].qual = quals ? (char*)quals[i] : 0; s[i].comment = 0;
	}
	orc_mem_process_pairs(opt, idx, n_processed, n, s, pes0, rg_id, pes_out, n_threads);
	size_t tot = 0;
	for (int i = 0; i < n; ++i) tot += strlen(s[i].sam);
	char *buf = malloc(tot + 1); size_t l = 0;
	for (int i = 0; i < n; ++i) { size_t k = strlen(s[i].sam); sam_off[i] = (int64_t)l; memcpy(buf + l, s[i].sam, k); l += k; free(s[i].sam); free(s[i].seq); }
	sam_off[n] = (int64_t)l; buf[l] = 0;
	free(s);
	return buf;
}

/* Exposure of the one container that is not upstream's (orc_mem.c: the chains of a read in a position-sorted array instead of klib's B-tree): every read through
 * both, on n_threads threads.  out[0] = reads whose chain lists differ, [1] = reads with more than 9 chains AND two chains at one position (the only reads that can
 * differ), [2] = reads with more than 9 chains, [3] = reads with two chains at one position, [4] = reads looked at. */
#include <pthread.h>
typedef struct { const orc_opt_t *opt; const orc_idx_t *idx; const uint8_t *seq; const int64_t *off; int r0, r1; int64_t c[4]; int32_t *which; } expo_t;
static void *expo_worker(void *p)
{
	expo_t *w = (expo_t*)p;
	for (int r = w->r0; r < w->r1; ++r) {
		int nc = 0, dup = 0;
		const int d = orc_chain_exposure(w->opt, w->idx, (int)(w->off[r + 1] - w->off[r]), w->seq + w->off[r], &nc, &dup);
		w->c[0] += d; w->c[1] += nc > 9 && dup; w->c[2] += nc > 9; w->c[3] += dup;
		if (w->which) w->which[r] = (d ? 1 : 0) | (nc > 9 && dup ? 2 : 0);
	}
	return 0;
}
void orc_api_chain_exposure(const orc_opt_t *opt, const orc_idx_t *idx, int n_reads, const uint8_t *seq, const int64_t *off, int n_threads, int64_t out[5], int32_t *which /* may be NULL: per read, bit 0 differs, bit 1 > 9 chains and a shared position */)
{
	if (n_threads < 1) n_threads = 1;
	if (n_threads > n_reads) n_threads = n_reads > 0 ? n_reads : 1;
	pthread_t *th = malloc(n_threads * sizeof(pthread_t)); expo_t *w = calloc(n_threads, sizeof(expo_t));
	for (int t = 0; t < n_threads; ++t) {
		w[t].opt = opt; w[t].idx = idx; w[t].seq = seq; w[t].off = off; w[t].which = which;
		w[t].r0 = (int)((int64_t)n_reads * t / n_threads); w[t].r1 = (int)((int64_t)n_reads * (t + 1) / n_threads);
		pthread_create(&th[t], 0, expo_worker, &w[t]);
	}
	out[0] = out[1] = out[2] = out[3] = 0; out[4] = n_reads;
	for (int t = 0; t < n_threads; ++t) { pthread_join(th[t], 0); for (int k = 0; k < 4; ++k) out[k] += w[t].c[k]; }
	free(th); free(w);
}
/* the container of mem_chain for the calls this thread makes (orc_align1 and the batch entry points run their workers on threads of their own: see ORC_CHAIN_KBTREE) */
void orc_api_set_chain_container(int kbtree) { orc_set_chain_container(kbtree); }

/* exposure of the other shared deviation (orc_ksw.c local_sw): on = 1 makes every orc_ksw_align2 call run a second time with E never opened from an F-raised H
 * and counts the calls whose result changes; out[0] = calls, out[1] = calls that differ (both since the process began) */
extern int orc_lazyf_count; extern uint64_t orc_lazyf_calls, orc_lazyf_differ;
void orc_api_lazyf(int on, uint64_t out[2]) { if (on >= 0) orc_lazyf_count = on; out[0] = orc_lazyf_calls; out[1] = orc_lazyf_differ; }
