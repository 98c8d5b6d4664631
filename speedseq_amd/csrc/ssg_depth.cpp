/*
 * ssg_depth.cpp -- ssg_depth_create / begin / push / finish / get / sums / text / end / free: coverage of records that lie in the record store (k_depth.h; the
 * program whose numbers it gives: `samtools depth' and `samtools bedcov' of the reference's samtools 1.3.1).  A push scans a chunk with the scan's own host code
 * (recs_scan_dev, ssg_bam_scan.cpp), decides on the device which records take part and adds them to the span's difference arrays; nothing is added before the
 * scan and the decision have succeeded, so a failed push leaves the counters as they were.  ssg_depth_finish turns the differences into counts with the tree's
 * exclusive sum (ssg_prim.h), read one entry further on.  A translation unit of its own: the machine code of the pinned kernels does not move (tools/isa_pin.py).
 */
#include <string>
#include <vector>
#include "ssg_rt.h"
#include "k_depth.h"
#include "ssg_prim.h"
#include "../../include/ssgpu.h"
#include "ssg_recs_int.h"

/* state: 0 no span; 1 a span that takes pushes (d_sd / d_cd: the differences); 2 finished (d_s / d_c: exclusive sums of n + 1 entries, the counts from entry 1) */
struct ssg_depth {
	ssg_recs *r; std::vector<ssg_bam_fop_t> prog; ssg_bam_fop_t *d_prog; int32_t min_baseq, tile;
	int state; int32_t tid; int64_t beg, end;
	uint32_t *d_sd, *d_cd, *d_s, *d_c;
	ssg_depth() : r(0), d_prog(0), min_baseq(0), tile(0), state(0), tid(0), beg(0), end(0), d_sd(0), d_cd(0), d_s(0), d_c(0) {}
};
static void depth_drop(ssg_depth *d)
{
	rt_free(d->d_sd); rt_free(d->d_cd); rt_free(d->d_s); rt_free(d->d_c);
	d->d_sd = d->d_cd = d->d_s = d->d_c = 0; d->state = 0;
}
static int depth_usable(const ssg_depth *d, const char *who)
{
	if (rt_device_count() < 1) { ssg_err_msg = "no HIP device visible: libssgpu has no CPU path"; return SSG_ENODEV; }
	if (!d) { ssg_err_msg = std::string(who) + ": no object"; return SSG_EINVAL; }
	return recs_usable(d->r, who);
}
/* [p0, p1) inside the finished span */
static int depth_range_ok(const ssg_depth *d, const char *who, int64_t p0, int64_t p1)
{
	if (d->state != 2) { ssg_err_msg = std::string(who) + ": no finished span (ssg_depth_begin, ssg_depth_push, ssg_depth_finish first)"; return SSG_EINVAL; }
	if (p0 < d->beg || p1 > d->end || p0 > p1) { ssg_err_msg = std::string(who) + ": positions " + std::to_string(p0) + " .. " + std::to_string(p1) + " are not inside the span " + std::to_string(d->beg) + " .. " + std::to_string(d->end); return SSG_EINVAL; }
	return 0;
}

extern "C" {

int ssg_depth_create(ssg_recs_t *r, const ssg_bam_fop_t *prog, int n_prog, int min_baseq, ssg_depth_t **out)
{
	if (rt_device_count() < 1) { ssg_err_msg = "no HIP device visible: libssgpu has no CPU path"; return SSG_ENODEV; }
	if (!r) { ssg_err_msg = "ssg_depth_create: no record store"; return SSG_EINVAL; }
	CHK(recs_usable(r, "ssg_depth_create"));
	if (!out) { ssg_err_msg = "ssg_depth_create: no place for the handle"; return SSG_EINVAL; }
	CHK(recs_prog_ok("ssg_depth_create: ", prog, n_prog));
	if (min_baseq < 0 || min_baseq > 255) { ssg_err_msg = "ssg_depth_create: min_baseq outside 0 .. 255"; return SSG_EINVAL; }
	ssg_depth *d = new ssg_depth();
	d->r = r; d->min_baseq = min_baseq; d->prog.assign(prog, prog + n_prog);
	/* SSG_DEPTH_TILE: the positions of the LDS tile of ssg_k_depth_accum (0: every add goes to global memory); the counters do not depend on it */
	const char *const t = getenv("SSG_DEPTH_TILE");
	d->tile = t && *t ? atoi(t) : 4095;
	if (d->tile < 0) d->tile = 0;
	if (d->tile > DEPTH_TILE_MAX) d->tile = DEPTH_TILE_MAX;
	d->d_prog = (ssg_bam_fop_t*)rt_malloc_raw(((size_t)n_prog + 1) * sizeof(ssg_bam_fop_t));
	int rc = d->d_prog ? 0 : SSG_ENOMEM;
	if (rc) ssg_err_msg = "device allocation failed: the filter program of ssg_depth_create";
	if (!rc && n_prog) rc = rt_h2d(d->d_prog, prog, (size_t)n_prog * sizeof(ssg_bam_fop_t));
	if (rc) { rt_free_raw(d->d_prog); delete d; return rc; }
	*out = d;
	return 0;
}

void ssg_depth_free(ssg_depth_t *d)
{
	if (!d) return;
	(void)rt_sync();
	depth_drop(d); rt_free_raw(d->d_prog);
	delete d;
}

int ssg_depth_begin(ssg_depth_t *d, int32_t tid, int64_t beg, int64_t end)
{
	CHK(depth_usable(d, "ssg_depth_begin"));
	if (d->state != 0) { ssg_err_msg = "ssg_depth_begin: a span is open (ssg_depth_end first)"; return SSG_EINVAL; }
	if (tid < 0 || beg < 0 || beg >= end || end > 0x7fffffffll) { ssg_err_msg = "ssg_depth_begin: tid < 0, or not 0 <= beg < end <= 2^31 - 1"; return SSG_EINVAL; }
	const size_t bytes = ((size_t)(end - beg) + 1) * 4;
	uint32_t *a = (uint32_t*)rt_malloc(bytes), *b = a ? (uint32_t*)rt_malloc(bytes) : 0;   /* (the arena: a command of many small spans asks the driver once) */
	int rc = a && b ? 0 : SSG_ENOMEM;
	if (rc) ssg_err_msg = "device allocation failed: the counters of a span of " + std::to_string(end - beg) + " positions";
	if (!rc) rc = rt_memset(a, 0, bytes);
	if (!rc) rc = rt_memset(b, 0, bytes);
	if (!rc) rc = rt_sync();
	if (rc) { rt_free(a); rt_free(b); return rc; }
	d->d_sd = a; d->d_cd = b; d->tid = tid; d->beg = beg; d->end = end; d->state = 1;
	return 0;
}

int ssg_depth_end(ssg_depth_t *d)
{
	CHK(depth_usable(d, "ssg_depth_end"));
	if (d->state == 0) { ssg_err_msg = "ssg_depth_end: no span is open"; return SSG_EINVAL; }
	CHK(rt_sync());
	depth_drop(d);
	return 0;
}

int ssg_depth_push(ssg_depth_t *d, uint32_t chunk_id, const uint64_t *hint, int64_t n_hints, uint64_t first, uint64_t *n_rec, uint64_t *n_used, uint64_t *n_later, uint64_t *descents, uint64_t *n_behind)
{
	const std::string who = "ssg_depth_push";
	CHK(depth_usable(d, "ssg_depth_push"));
	if (!n_rec || !n_used || !n_later || !descents) { ssg_err_msg = who + ": no place for the numbers of records"; return SSG_EINVAL; }
	*n_rec = *n_used = *n_later = *descents = 0;
	if (n_behind) *n_behind = 0;
	if (d->state != 1) { ssg_err_msg = who + (d->state == 0 ? ": no span is open (ssg_depth_begin first)" : ": the span is finished (ssg_depth_end, ssg_depth_begin first)"); return SSG_EINVAL; }
	ssg_recs *const r = d->r;
	if (r->ordered) { ssg_err_msg = who + ": refused while an order is declared: ssg_recs_reopen first"; return SSG_EINVAL; }
	recs_scan_dev_t s;
	CHK(recs_scan_dev(r, "ssg_depth_push", chunk_id, hint, n_hints, first, ~(uint64_t)0, true, n_rec, s));
	const uint64_t n = *n_rec;
	if (n == 0) return 0;
	const uint64_t grid = (n + 255) / 256;   /* (below 2^31: the scan has checked it) */
	dbuf<uint8_t> d_use((size_t)n); dbuf<uint32_t> d_idx((size_t)n), d_kept((size_t)n); dbuf<unsigned long long> d_cnt(5);
	if (!d_use.ok() || !d_idx.ok() || !d_kept.ok() || !d_cnt.ok()) { ssg_err_msg = "device allocation failed: the decisions of ssg_depth_push"; return SSG_ENOMEM; }
	CHK(rt_memset(d_cnt.p, 0, 40)); CHK(rt_memset(d_cnt.p + 3, 0xff, 8));
	const uint8_t *const d_chunk = r->d_chunk[chunk_id];
	SSG_LAUNCH(ssg_k_depth_decide, grid, 256, 0, d_chunk, (const uint64_t*)s.loc.p, (const uint64_t*)s.key.p, (const ssg_bam_ent_t*)s.ent.p, (int64_t)n, (const ssg_bam_fop_t*)d->d_prog, (int32_t)d->prog.size(),
	           d->tid, (int32_t)d->beg, (int32_t)d->end, d->min_baseq, d_use.p, d_idx.p, d_cnt.p);
	uint64_t m = 0;
	CHK(prim_select((const uint32_t*)d_idx.p, (const uint8_t*)d_use.p, (int64_t)n, d_kept.p, &m));   /* (ends in a download: the decisions are taken) */
	unsigned long long cnt[5] = { 0, 0, 0, 0, 0 }; CHK(d_cnt.down(cnt, 5));
	if (cnt[3] != ~0ull) { ssg_err_msg = who + ": malformed record at offset " + std::to_string(cnt[3]) + ": 32 + l_qname + 4 n_cigar + (l_seq + 1) / 2 + l_seq exceeds block_size"; return SSG_EIO; }
	if (m != cnt[0] || m > n) { ssg_err_msg = who + ": the selection returned " + std::to_string(m) + " records, " + std::to_string(cnt[0]) + " were decided"; return SSG_EHIP; }
	/* every stage that can fail has succeeded: the adds */
	if (m > 0) {
		SSG_LAUNCH(ssg_k_depth_accum, (m + 255) / 256, 256, d->tile > 0 ? 2 * ((size_t)d->tile + 1) * 4 : 0, d_chunk, (const uint64_t*)s.loc.p, (const ssg_bam_ent_t*)s.ent.p, (const uint32_t*)d_kept.p, (uint32_t)m,
		           (int32_t)d->beg, (int32_t)d->end, d->min_baseq, d->tile, d->d_sd, d->d_cd);
		CHK(rt_sync());
	}
	*n_used = m; *n_later = cnt[1]; *descents = cnt[2];
	if (n_behind) *n_behind = cnt[4];
	return 0;
}

int ssg_depth_finish(ssg_depth_t *d)
{
	CHK(depth_usable(d, "ssg_depth_finish"));
	if (d->state != 1) { ssg_err_msg = d->state == 0 ? "ssg_depth_finish: no span is open" : "ssg_depth_finish: the span is finished already"; return SSG_EINVAL; }
	const int64_t n1 = d->end - d->beg + 1;
	uint32_t *a = (uint32_t*)rt_malloc((size_t)n1 * 4), *b = a ? (uint32_t*)rt_malloc((size_t)n1 * 4) : 0;
	if (!a || !b) { rt_free(a); rt_free(b); ssg_err_msg = "device allocation failed: the sums of a span of " + std::to_string(n1 - 1) + " positions"; return SSG_ENOMEM; }
	/* (the differences are taken modulo 2^32, as the counts are: the sum of n + 1 entries, read from entry 1, is the inclusive sum of the first n) */
	int rc = prim_exsum<uint32_t, uint32_t>(d->d_sd, a, n1);
	if (!rc) rc = prim_exsum<uint32_t, uint32_t>(d->d_cd, b, n1);
	if (!rc) rc = rt_sync();
	if (rc) { rt_free(a); rt_free(b); return rc; }
	rt_free(d->d_sd); rt_free(d->d_cd); d->d_sd = d->d_cd = 0;
	d->d_s = a; d->d_c = b; d->state = 2;
	return 0;
}

int ssg_depth_get(ssg_depth_t *d, int64_t p0, int64_t p1, uint32_t *span_out, uint32_t *cov_out)
{
	CHK(depth_usable(d, "ssg_depth_get"));
	CHK(depth_range_ok(d, "ssg_depth_get", p0, p1));
	if (p0 == p1) return 0;
	if (!span_out || !cov_out) { ssg_err_msg = "ssg_depth_get: no span_out[] / cov_out[]"; return SSG_EINVAL; }
	CHK(rt_d2h(span_out, d->d_s + 1 + (p0 - d->beg), (size_t)(p1 - p0) * 4));
	CHK(rt_d2h(cov_out, d->d_c + 1 + (p0 - d->beg), (size_t)(p1 - p0) * 4));
	return 0;
}

int ssg_depth_sums(ssg_depth_t *d, const int64_t *reg, int64_t n_reg, const uint32_t *thr, int n_thr, uint64_t *out)
{
	const std::string who = "ssg_depth_sums";
	CHK(depth_usable(d, "ssg_depth_sums"));
	if (d->state != 2) { ssg_err_msg = who + ": no finished span (ssg_depth_begin, ssg_depth_push, ssg_depth_finish first)"; return SSG_EINVAL; }
	if (n_reg < 0 || (n_reg > 0 && (!reg || !out))) { ssg_err_msg = who + ": n_reg < 0, or no reg[] / out[]"; return SSG_EINVAL; }
	if (n_thr < 0 || n_thr > DEPTH_THR_MAX || (n_thr > 0 && !thr)) { ssg_err_msg = who + ": n_thr outside 0 .. " + std::to_string(DEPTH_THR_MAX) + ", or no thr[]"; return SSG_EINVAL; }
	std::vector<depth_seg_t> seg;
	for (int64_t k = 0; k < n_reg; ++k) {
		const int64_t b = reg[2 * k], e = reg[2 * k + 1];
		if (b >= e || b < d->beg || e > d->end) { ssg_err_msg = who + ": pair " + std::to_string(k) + " (" + std::to_string(b) + ", " + std::to_string(e) + ") has beg >= end or is not inside the span " + std::to_string(d->beg) + " .. " + std::to_string(d->end); return SSG_EINVAL; }
		for (int64_t p = b; p < e; p += DEPTH_SEG) { depth_seg_t g; g.beg = p - d->beg; g.end = std::min<int64_t>(p + DEPTH_SEG, e) - d->beg; g.pair = k; seg.push_back(g); }
	}
	if (n_reg == 0) return 0;
	const size_t row = 2 + (size_t)n_thr, n_seg = seg.size();
	dbuf<depth_seg_t> d_seg(n_seg); dbuf<uint32_t> d_thr((size_t)n_thr + 1); dbuf<unsigned long long> d_out((size_t)n_reg * row);
	if (!d_seg.ok() || !d_thr.ok() || !d_out.ok()) { ssg_err_msg = "device allocation failed: the segments of ssg_depth_sums"; return SSG_ENOMEM; }
	CHK(d_seg.up(seg.data(), n_seg));
	if (n_thr) CHK(d_thr.up(thr, (size_t)n_thr));
	CHK(d_out.zero());
	SSG_LAUNCH(ssg_k_depth_sums, (n_seg + 3) / 4, 256, 0, (const uint32_t*)(d->d_s + 1), (const uint32_t*)(d->d_c + 1), d->end - d->beg, (const depth_seg_t*)d_seg.p, (int64_t)n_seg,
	           (const uint32_t*)d_thr.p, (int32_t)n_thr, d_out.p, n_reg);
	CHK(rt_sync());
	static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit sums");
	return rt_d2h(out, d_out.p, (size_t)n_reg * row * 8);
}

int ssg_depth_text(ssg_depth_t *d, const char *name, int64_t p0, int64_t p1, int all, uint8_t *out, uint64_t cap, uint64_t *len)
{
	const std::string who = "ssg_depth_text";
	CHK(depth_usable(d, "ssg_depth_text"));
	if (!len) { ssg_err_msg = who + ": no place for the text's length"; return SSG_EINVAL; }
	*len = 0;
	CHK(depth_range_ok(d, "ssg_depth_text", p0, p1));
	const size_t nl = name ? strlen(name) : 0;
	if (nl == 0 || nl > 65535) { ssg_err_msg = who + ": no name, or one of more than 65535 bytes"; return SSG_EINVAL; }
	if (!out && cap) { ssg_err_msg = who + ": no out[]"; return SSG_EINVAL; }
	const int64_t n = p1 - p0;
	if (n == 0) return 0;
	dbuf<uint32_t> d_len((size_t)n + 1); dbuf<uint64_t> d_off((size_t)n + 1); dbuf<uint8_t> d_name(nl);
	if (!d_len.ok() || !d_off.ok() || !d_name.ok()) { ssg_err_msg = "device allocation failed: the line lengths of ssg_depth_text"; return SSG_ENOMEM; }
	CHK(d_name.up((const uint8_t*)name, nl));
	CHK(rt_memset(d_len.p + n, 0, 4));   /* (one more: the sum's last value is the total) */
	const uint64_t grid = ((uint64_t)n + 255) / 256;
	SSG_LAUNCH(ssg_k_depth_lens, grid, 256, 0, (const uint32_t*)(d->d_s + 1), (const uint32_t*)(d->d_c + 1), p0 - d->beg, n, d->beg, (uint32_t)nl, (int32_t)(all != 0), d_len.p);
	CHK((prim_exsum<uint32_t, uint64_t>(d_len.p, d_off.p, n + 1)));
	CHK(rt_sync());
	uint64_t total = 0; CHK(rt_d2h(&total, d_off.p + n, 8));
	*len = total;
	if (total > cap) {
		if (!out && cap == 0) return 0;   /* the sizing form */
		ssg_err_msg = who + ": " + std::to_string(total) + " bytes of text, room for " + std::to_string(cap); return SSG_EOVERFLOW;
	}
	if (total == 0) return 0;
	dbuf<uint8_t> d_out((size_t)total);
	if (!d_out.ok()) { ssg_err_msg = "device allocation failed: the text of ssg_depth_text"; return SSG_ENOMEM; }
	SSG_LAUNCH(ssg_k_depth_text, grid, 256, 0, (const uint32_t*)(d->d_c + 1), p0 - d->beg, n, d->beg, (const uint8_t*)d_name.p, (uint32_t)nl, (const uint32_t*)d_len.p, (const uint64_t*)d_off.p, d_out.p, total);
	CHK(rt_sync());
	return rt_d2h(out, d_out.p, (size_t)total);
}

} /* extern "C" */
