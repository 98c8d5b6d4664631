/*
 * ssg_markdup.cpp -- ssg_markdup_create / push / finish / get / apply / free: Picard's duplicate rule for records that lie in the record store (k_markdup.h; the
 * rule: include/ssgpu.h).  A push scans a chunk with the scan's own host code (recs_scan_dev, ssg_bam_scan.cpp), leaves one entry per record and the names of
 * the paired records in device memory of the object's own that counts against the store's capacity, and releases the chunk.  Every array of a push is a
 * temporary until the entries are in place: a failed push leaves the object as it was.  The decision (finish) is the mate join of ssg_b2f.cpp, then for pairs and
 * for fragments stable LSD radix passes over the key bits in use (ssg_prim.h), a boundary flag per element and a running maximum of (group, score, ~ordinal):
 * no walk is as long as a group.  The second pass (apply) scans a chunk again, checks it against the entries, patches the flag bytes and compacts the kept
 * records as ssg_recs_select does.  A translation unit of its own: the machine code of the pinned kernels does not move (tools/isa_pin.py).
 */
#include <algorithm>
#include <string>
#include <vector>
#include "ssg_rt.h"
#include "k_markdup.h"
#include "ssg_prim.h"
#include "../../include/ssgpu.h"
#include "ssg_recs_int.h"

/* a device array that grows by appends; its bytes count against the store's capacity */
struct md_arr_t {
	uint8_t *p; size_t used, cap;
	md_arr_t() : p(0), used(0), cap(0) {}
};

struct ssg_markdup {
	ssg_recs *r; int hash_bits; int32_t n_rg;
	uint8_t *d_ids; uint32_t *d_idoff; uint16_t *d_lib;   /* the @RG ids one behind the other, n_rg + 1 offsets, their libraries */
	md_arr_t ents, names;                                  /* md_ent_t per ordinal; the names of the paired records */
	uint64_t n;                                            /* records pushed */
	int state;                                             /* 0 takes pushes; 1 decided */
	uint32_t *d_bitmap; size_t bitmap_bytes;               /* a duplicate bit per ordinal */
	uint64_t a_ord;                                        /* the running ordinal of the second pass */
	ssg_markdup() : r(0), hash_bits(64), n_rg(0), d_ids(0), d_idoff(0), d_lib(0), n(0), state(0), d_bitmap(0), bitmap_bytes(0), a_ord(0) {}
};

static int md_usable(const ssg_markdup *m, const char *who)
{
	if (rt_device_count() < 1) { ssg_err_msg = "no HIP device visible: libssgpu has no CPU path"; return SSG_ENODEV; }
	if (!m) { ssg_err_msg = std::string(who) + ": no object"; return SSG_EINVAL; }
	return recs_usable(m->r, who);
}
static bool md_fits(const ssg_recs *r, size_t more) { return more <= r->cap && r->bytes <= r->cap - more; }
/* room for `need' bytes in all; what the array holds stays */
static int md_reserve(ssg_recs *r, md_arr_t &a, size_t need, const char *what)
{
	if (need <= a.cap) return 0;
	size_t cap = std::max(need, a.cap + a.cap / 2);
	if (!md_fits(r, cap - a.cap)) cap = need;
	uint8_t *p = md_fits(r, cap - a.cap) ? (uint8_t*)rt_malloc_raw(cap + 16) : 0;
	if (!p) { ssg_err_msg = std::string("device allocation failed: ") + what + " (" + std::to_string(need) + " bytes; they count against the store's capacity)"; return SSG_ENOMEM; }
	int rc = rt_d2d(p, a.p, a.used);
	if (!rc) rc = rt_sync();
	if (rc) { rt_free_raw(p); return rc; }
	rt_free_raw(a.p);
	r->bytes += cap - a.cap;
	a.p = p; a.cap = cap;
	return 0;
}
static void md_drop(ssg_recs *r, md_arr_t &a) { rt_free_raw(a.p); r->bytes -= a.cap; a.p = 0; a.used = a.cap = 0; }
static int md_bits_of(uint64_t v) { int b = 0; while (b < 64 && (v >> b)) ++b; return b; }

struct md_pass_t { int32_t w; int b0, b1; };
/* the decision over m elements: d_idx (0 .. m - 1 on entry) is sorted by the passes' key bits, groups are found, the best of each is kept */
static int md_decide(const md_key_t *d_key, dbuf<uint32_t> &d_idx, uint64_t m, const std::vector<md_pass_t> &passes, uint64_t n, uint32_t *d_bitmap, unsigned long long *c_pairs, unsigned long long *c_frags)
{
	if (m == 0) return 0;
	const uint64_t grid = (m + 255) / 256;
	{
		dbuf<uint64_t> d_k1((size_t)m), d_k2((size_t)m); dbuf<uint32_t> d_i2((size_t)m);
		if (!d_k1.ok() || !d_k2.ok() || !d_i2.ok()) { ssg_err_msg = "device allocation failed: the sort keys of ssg_markdup_finish"; return SSG_ENOMEM; }
		for (const md_pass_t &ps : passes) {
			if (ps.b1 <= ps.b0) continue;
			SSG_LAUNCH(ssg_k_md_word, grid, 256, 0, d_key, (const uint32_t*)d_idx.p, (uint32_t)m, ps.w, d_k1.p);
			CHK(prim_sort_pairs(d_k1.p, d_k2.p, d_idx.p, d_i2.p, (int64_t)m, ps.b0, ps.b1));   /* stable: what the earlier passes ordered stays ordered */
			d_idx.swap(d_i2);
		}
		CHK(rt_sync());
	}
	dbuf<uint32_t> d_head((size_t)m), d_before((size_t)m); dbuf<md_w128_t> d_w((size_t)m), d_run((size_t)m), d_best((size_t)m);
	if (!d_head.ok() || !d_before.ok() || !d_w.ok() || !d_run.ok() || !d_best.ok()) { ssg_err_msg = "device allocation failed: the groups of ssg_markdup_finish"; return SSG_ENOMEM; }
	SSG_LAUNCH(ssg_k_md_heads, grid, 256, 0, d_key, (const uint32_t*)d_idx.p, (uint32_t)m, d_head.p);
	CHK((prim_exsum<uint32_t, uint32_t>(d_head.p, d_before.p, (int64_t)m)));
	SSG_LAUNCH(ssg_k_md_pack, grid, 256, 0, d_key, (const uint32_t*)d_idx.p, (const uint32_t*)d_head.p, (const uint32_t*)d_before.p, (uint32_t)m, d_w.p);
	CHK(prim_scan_max((const md_w128_t*)d_w.p, d_run.p, (int64_t)m));
	SSG_LAUNCH(ssg_k_md_best, grid, 256, 0, (const md_w128_t*)d_run.p, (const uint32_t*)d_head.p, (const uint32_t*)d_before.p, (uint32_t)m, d_best.p);
	SSG_LAUNCH(ssg_k_md_mark, grid, 256, 0, d_key, (const uint32_t*)d_idx.p, (const uint32_t*)d_head.p, (const uint32_t*)d_before.p, (const md_w128_t*)d_best.p, (uint32_t)m, n, d_bitmap, c_pairs, c_frags);
	return rt_sync();
}

extern "C" {

int ssg_markdup_create(ssg_recs_t *r, const char *const *rg, const uint16_t *lib_of_rg, int n_rg, int hash_bits, ssg_markdup_t **out)
{
	if (!r) { ssg_err_msg = "ssg_markdup_create: no record store"; return SSG_EINVAL; }
	CHK(recs_usable(r, "ssg_markdup_create"));
	if (!out) { ssg_err_msg = "ssg_markdup_create: no place for the handle"; return SSG_EINVAL; }
	if (n_rg < 0 || (n_rg > 0 && (!rg || !lib_of_rg))) { ssg_err_msg = "ssg_markdup_create: n_rg < 0, or no rg[] / lib_of_rg[]"; return SSG_EINVAL; }
	if (hash_bits < 0 || hash_bits > 64) { ssg_err_msg = "ssg_markdup_create: hash_bits outside 0 .. 64"; return SSG_EINVAL; }
	std::vector<uint8_t> ids; std::vector<uint32_t> off(1, 0);
	for (int g = 0; g < n_rg; ++g) {
		if (!rg[g] || !rg[g][0]) { ssg_err_msg = "ssg_markdup_create: read group id " + std::to_string(g) + " is NULL or empty"; return SSG_EINVAL; }
		ids.insert(ids.end(), (const uint8_t*)rg[g], (const uint8_t*)rg[g] + strlen(rg[g]));
		if (ids.size() > 0x7fffffffu) { ssg_err_msg = "ssg_markdup_create: the read group ids exceed 2^31 bytes"; return SSG_EINVAL; }
		off.push_back((uint32_t)ids.size());
	}
	ssg_markdup *m = new ssg_markdup();
	m->r = r; m->hash_bits = hash_bits; m->n_rg = n_rg;
	m->d_ids = (uint8_t*)rt_malloc_raw(ids.size() + 16); m->d_idoff = (uint32_t*)rt_malloc_raw(off.size() * 4); m->d_lib = (uint16_t*)rt_malloc_raw((size_t)n_rg * 2 + 16);
	int rc = m->d_ids && m->d_idoff && m->d_lib ? 0 : SSG_ENOMEM;
	if (rc) ssg_err_msg = "device allocation failed: the read group ids of ssg_markdup_create";
	if (!rc) rc = rt_h2d(m->d_ids, ids.data(), ids.size());
	if (!rc) rc = rt_h2d(m->d_idoff, off.data(), off.size() * 4);
	if (!rc && n_rg) rc = rt_h2d(m->d_lib, lib_of_rg, (size_t)n_rg * 2);
	if (rc) { rt_free_raw(m->d_ids); rt_free_raw(m->d_idoff); rt_free_raw(m->d_lib); delete m; return rc; }
	*out = m;
	return 0;
}

void ssg_markdup_free(ssg_markdup_t *m)
{
	if (!m) return;
	(void)rt_sync();
	md_drop(m->r, m->ents); md_drop(m->r, m->names);
	rt_free_raw(m->d_bitmap); m->r->bytes -= m->bitmap_bytes;
	rt_free_raw(m->d_ids); rt_free_raw(m->d_idoff); rt_free_raw(m->d_lib);
	delete m;
}

int ssg_markdup_push(ssg_markdup_t *m, uint32_t chunk_id, const uint64_t *hint, int64_t n_hints, uint64_t first, uint64_t *n_rec)
{
	const std::string who = "ssg_markdup_push";
	CHK(md_usable(m, "ssg_markdup_push"));
	if (!n_rec) { ssg_err_msg = who + ": no place for the number of records"; return SSG_EINVAL; }
	*n_rec = 0;
	if (m->state != 0) { ssg_err_msg = who + ": the object is finished (ssg_markdup_finish was called)"; return SSG_EINVAL; }
	ssg_recs *const r = m->r;
	if (r->ordered) { ssg_err_msg = who + ": refused while an order is declared: ssg_recs_reopen first"; return SSG_EINVAL; }
	recs_scan_dev_t s;
	CHK(recs_scan_dev(r, "ssg_markdup_push", chunk_id, hint, n_hints, first, ~(uint64_t)0, true, n_rec, s));
	const uint64_t n = *n_rec;
	if (n == 0) return ssg_recs_release(r, chunk_id);
	if (m->n + n > MD_ORD_MAX) { ssg_err_msg = who + ": more than 2^32 - 16 records in one stream"; return SSG_EINVAL; }
	const uint8_t *const d_chunk = r->d_chunk[chunk_id];
	dbuf<md_ent_t> d_ent((size_t)n); dbuf<uint32_t> d_nlen((size_t)n + 1); dbuf<uint64_t> d_noff((size_t)n + 1); dbuf<unsigned long long> d_bad(1);
	if (!d_ent.ok() || !d_nlen.ok() || !d_noff.ok() || !d_bad.ok()) { ssg_err_msg = "device allocation failed: the entries of ssg_markdup_push"; return SSG_ENOMEM; }
	CHK(rt_memset(d_bad.p, 0xff, 8)); CHK(rt_memset(d_nlen.p + n, 0, 4));   /* (one more: the sum's last value is the total) */
	SSG_LAUNCH(ssg_k_md_ends, (n + 255) / 256, 256, 0, d_chunk, (const uint64_t*)s.loc.p, (uint32_t)n, (const uint8_t*)m->d_ids, (const uint32_t*)m->d_idoff, (const uint16_t*)m->d_lib, m->n_rg,
	           d_ent.p, d_nlen.p, d_bad.p);
	CHK((prim_exsum<uint32_t, uint64_t>(d_nlen.p, d_noff.p, (int64_t)n + 1)));
	CHK(rt_sync());
	unsigned long long bad = 0; CHK(d_bad.down(&bad, 1));
	if (bad != ~0ull) { ssg_err_msg = who + ": malformed record at offset " + std::to_string(bad) + ": 32 + l_qname + 4 n_cigar + (l_seq + 1) / 2 + l_seq exceeds block_size"; return SSG_EIO; }
	uint64_t nb = 0; CHK(rt_d2h(&nb, d_noff.p + n, 8));
	if (nb > 255 * n) { ssg_err_msg = who + ": the names' sum exceeds what the records can hold"; return SSG_EHIP; }
	dbuf<uint8_t> d_names((size_t)nb + 16);
	if (!d_names.ok()) { ssg_err_msg = "device allocation failed: the names of ssg_markdup_push"; return SSG_ENOMEM; }
	SSG_LAUNCH(ssg_k_md_score, (n + 15) / 16, 256, 0, d_chunk, (const uint64_t*)s.loc.p, (uint32_t)n, (const uint64_t*)d_noff.p, (uint64_t)m->names.used, d_ent.p, d_names.p, nb);
	const size_t need_e = (size_t)(m->n + n) * sizeof(md_ent_t), need_n = m->names.used + (size_t)nb;
	if (!md_fits(r, (need_e > m->ents.cap ? need_e - m->ents.cap : 0) + (need_n > m->names.cap ? need_n - m->names.cap : 0))) {   /* (before either grows: a refusal leaves the store's sum as it was) */
		ssg_err_msg = "device allocation failed: the entries and names of ssg_markdup_push would exceed the store's capacity"; return SSG_ENOMEM;
	}
	CHK(md_reserve(r, m->ents, need_e, "the entries of ssg_markdup_push"));
	CHK(md_reserve(r, m->names, m->names.used + (size_t)nb, "the names of ssg_markdup_push"));
	CHK(rt_d2d(m->ents.p + m->ents.used, d_ent.p, (size_t)n * sizeof(md_ent_t)));
	CHK(rt_d2d(m->names.p + m->names.used, d_names.p, (size_t)nb));
	CHK(rt_sync());
	/* the entries are in place behind the ones that count: the chunk goes, then they count */
	CHK(ssg_recs_release(r, chunk_id));
	m->n += n; m->ents.used += (size_t)n * sizeof(md_ent_t); m->names.used += (size_t)nb;
	return 0;
}

int ssg_markdup_finish(ssg_markdup_t *m, uint64_t *counts)
{
	const std::string who = "ssg_markdup_finish";
	CHK(md_usable(m, "ssg_markdup_finish"));
	if (!counts) { ssg_err_msg = who + ": no place for the counts"; return SSG_EINVAL; }
	if (m->state != 0) { ssg_err_msg = who + ": the object is finished already"; return SSG_EINVAL; }
	for (int k = 0; k < SSG_MD_N; ++k) counts[k] = 0;
	ssg_recs *const r = m->r;
	const uint64_t n = m->n;
	if (n == 0) { m->state = 1; return 0; }
	const size_t bm_bytes = (size_t)((n + 31) / 32) * 4;
	uint32_t *d_bitmap = md_fits(r, bm_bytes) ? (uint32_t*)rt_malloc_raw(bm_bytes + 16) : 0;
	struct own_t { uint32_t *&p; ~own_t() { rt_free_raw(p); } } own = { d_bitmap };
	if (!d_bitmap) { ssg_err_msg = "device allocation failed: the bitmap of ssg_markdup_finish (" + std::to_string(bm_bytes) + " bytes; they count against the store's capacity)"; return SSG_ENOMEM; }
	CHK(rt_memset(d_bitmap, 0, bm_bytes));
	const md_ent_t *const d_ent = (const md_ent_t*)m->ents.p;
	const uint64_t grid = (n + 255) / 256;
	dbuf<unsigned long long> d_cnt(SSG_MD_N), d_or(4); dbuf<uint32_t> d_flags(1), d_idx((size_t)n), d_mate((size_t)n);
	uint64_t n_pairs = 0;
	unsigned long long bits[4] = { 0, 0, 0, 0 };
	{
		dbuf<uint8_t> d_selp((size_t)n), d_selt((size_t)n); dbuf<uint32_t> d_tpos((size_t)n);
		if (!d_cnt.ok() || !d_or.ok() || !d_flags.ok() || !d_idx.ok() || !d_mate.ok() || !d_selp.ok() || !d_selt.ok() || !d_tpos.ok()) { ssg_err_msg = "device allocation failed: the classes of ssg_markdup_finish"; return SSG_ENOMEM; }
		CHK(d_cnt.zero()); CHK(d_or.zero()); CHK(d_flags.zero());
		SSG_LAUNCH(ssg_k_md_classes, grid, 256, 0, d_ent, (uint32_t)n, d_selp.p, d_selt.p, d_idx.p, d_mate.p, d_cnt.p);
		SSG_LAUNCH(ssg_k_md_bits, std::min<uint64_t>(grid, 1024), 256, 0, d_ent, n, d_or.p);
		CHK(rt_sync());
		CHK(d_or.down(bits, 4));
		const int ub = md_bits_of(bits[0]), tb = md_bits_of(bits[1] & 0xffffffffu), lb = md_bits_of(bits[2] & 0xffffu);
		/* the mate join */
		uint64_t mp = 0;
		dbuf<uint32_t> d_ppos((size_t)n);
		if (!d_ppos.ok()) { ssg_err_msg = "device allocation failed: the paired records of ssg_markdup_finish"; return SSG_ENOMEM; }
		CHK(prim_select((const uint32_t*)d_idx.p, (const uint8_t*)d_selp.p, (int64_t)n, d_ppos.p, &mp));
		if (mp > n) { ssg_err_msg = who + ": the selection returned more records than it was given"; return SSG_EHIP; }
		if (mp > 0) {
			const uint64_t pgrid = (mp + 255) / 256;
			dbuf<uint64_t> d_key((size_t)mp), d_skey((size_t)mp); dbuf<uint32_t> d_spos((size_t)mp), d_own((size_t)mp); dbuf<uint8_t> d_owner((size_t)mp);
			if (!d_key.ok() || !d_skey.ok() || !d_spos.ok() || !d_own.ok() || !d_owner.ok()) { ssg_err_msg = "device allocation failed: the name keys of ssg_markdup_finish"; return SSG_ENOMEM; }
			SSG_LAUNCH(ssg_k_md_pkeys, pgrid, 256, 0, d_ent, (const uint32_t*)d_ppos.p, (uint32_t)mp, (uint32_t)n, (int32_t)m->hash_bits, d_key.p);
			CHK(prim_sort_pairs(d_key.p, d_skey.p, d_ppos.p, d_spos.p, (int64_t)mp, 0, 64));   /* stable: equal hashes stay in ordinal order */
			SSG_LAUNCH(ssg_k_md_join, pgrid, 256, 0, d_ent, (const uint8_t*)m->names.p, (uint64_t)m->names.used, (const uint64_t*)d_skey.p, (const uint32_t*)d_spos.p, (uint32_t)mp, (uint32_t)n, d_mate.p, d_flags.p);
			CHK(rt_sync());
			uint32_t fl = 0; CHK(d_flags.down(&fl, 1));
			if (fl & 2u) { ssg_err_msg = who + ": the sort returned a position outside the records, or an entry's name lies outside the names"; return SSG_EHIP; }
			if (fl & 1u) { ssg_err_msg = who + ": more than " + std::to_string(SSG_MARKDUP_RUN_MAX) + " paired records share one name hash of " + std::to_string(m->hash_bits) + " bits"; return SSG_ERANGE; }
			SSG_LAUNCH(ssg_k_md_owners, pgrid, 256, 0, (const uint32_t*)d_spos.p, (uint32_t)mp, (uint32_t)n, (const uint32_t*)d_mate.p, d_owner.p);
			CHK(prim_select((const uint32_t*)d_spos.p, (const uint8_t*)d_owner.p, (int64_t)mp, d_own.p, &n_pairs));
			if (2 * n_pairs > mp) { ssg_err_msg = who + ": more pairs than half the paired records"; return SSG_EHIP; }
			if (n_pairs > 0) {
				dbuf<md_key_t> d_pk((size_t)n_pairs); dbuf<uint32_t> d_pidx((size_t)n_pairs);
				if (!d_pk.ok() || !d_pidx.ok()) { ssg_err_msg = "device allocation failed: the pair list of ssg_markdup_finish"; return SSG_ENOMEM; }
				SSG_LAUNCH(ssg_k_md_pairs, (n_pairs + 255) / 256, 256, 0, d_ent, (const uint32_t*)d_mate.p, (const uint32_t*)d_own.p, (uint32_t)n_pairs, (uint32_t)n, d_pk.p, d_pidx.p);
				const std::vector<md_pass_t> passes = { { 3, 0, lb ? 18 + lb : 2 }, { 2, 0, tb }, { 2, 32, 32 + tb }, { 1, 0, ub }, { 0, 0, ub } };
				CHK(md_decide(d_pk.p, d_pidx, n_pairs, passes, n, d_bitmap, d_cnt.p + SSG_MD_DUP_PAIRED, (unsigned long long*)0));
			}
		}
		/* the fragments, among all the taking-part records of their end key */
		uint64_t mt = 0;
		CHK(prim_select((const uint32_t*)d_idx.p, (const uint8_t*)d_selt.p, (int64_t)n, d_tpos.p, &mt));
		if (mt > n) { ssg_err_msg = who + ": the selection returned more records than it was given"; return SSG_EHIP; }
		if (mt > 0) {
			dbuf<md_key_t> d_fk((size_t)mt); dbuf<uint32_t> d_fidx((size_t)mt);
			if (!d_fk.ok() || !d_fidx.ok()) { ssg_err_msg = "device allocation failed: the end keys of ssg_markdup_finish"; return SSG_ENOMEM; }
			SSG_LAUNCH(ssg_k_md_frags, (mt + 255) / 256, 256, 0, d_ent, (const uint32_t*)d_tpos.p, (uint32_t)mt, (uint32_t)n, d_fk.p, d_fidx.p);
			const std::vector<md_pass_t> passes = { { 3, 0, lb ? 2 + lb : 1 }, { 2, 0, tb }, { 0, 0, ub } };
			CHK(md_decide(d_fk.p, d_fidx, mt, passes, n, d_bitmap, (unsigned long long*)0, d_cnt.p + SSG_MD_DUP_FRAGMENTS));
		}
	}
	CHK(rt_sync());
	unsigned long long c[SSG_MD_N]; CHK(d_cnt.down(c, SSG_MD_N));
	for (int k = 0; k < SSG_MD_N; ++k) counts[k] = c[k];
	counts[SSG_MD_RECORDS] = n; counts[SSG_MD_PAIRS] = n_pairs; counts[SSG_MD_UNMATCHED] = counts[SSG_MD_PAIRED] - 2 * n_pairs;
	/* decided: the bitmap stays and counts, the names go */
	m->d_bitmap = d_bitmap; d_bitmap = 0; m->bitmap_bytes = bm_bytes; r->bytes += bm_bytes;
	md_drop(r, m->names);
	m->state = 1;
	return 0;
}

int ssg_markdup_get(ssg_markdup_t *m, uint64_t ord0, uint64_t n, uint8_t *dup)
{
	CHK(md_usable(m, "ssg_markdup_get"));
	if (m->state != 1) { ssg_err_msg = "ssg_markdup_get: nothing is decided yet: ssg_markdup_finish first"; return SSG_EINVAL; }
	if (ord0 > m->n || n > m->n - ord0) { ssg_err_msg = "ssg_markdup_get: ordinals " + std::to_string(ord0) + " .. + " + std::to_string(n) + " run past the " + std::to_string(m->n) + " records"; return SSG_EINVAL; }
	if (n == 0) return 0;
	if (!dup) { ssg_err_msg = "ssg_markdup_get: no dup[]"; return SSG_EINVAL; }
	CHK(rt_sync());
	const uint64_t w0 = ord0 >> 5, w1 = (ord0 + n + 31) >> 5;
	std::vector<uint32_t> w((size_t)(w1 - w0));
	CHK(rt_d2h(w.data(), m->d_bitmap + w0, (size_t)(w1 - w0) * 4));
	for (uint64_t k = 0; k < n; ++k) { const uint64_t o = ord0 + k; dup[k] = (uint8_t)(w[(size_t)((o >> 5) - w0)] >> (o & 31) & 1u); }
	return 0;
}

int ssg_markdup_apply(ssg_markdup_t *m, uint32_t chunk_id, const uint64_t *hint, int64_t n_hints, uint64_t first, int remove, uint64_t cap,
                      uint64_t *n_rec, uint64_t *n_kept, uint64_t *loc, ssg_bam_ent_t *ent)
{
	const std::string who = "ssg_markdup_apply";
	CHK(md_usable(m, "ssg_markdup_apply"));
	if (!n_rec || !n_kept) { ssg_err_msg = who + ": no place for the number of records"; return SSG_EINVAL; }
	*n_rec = *n_kept = 0;
	if (m->state != 1) { ssg_err_msg = who + ": nothing is decided yet: ssg_markdup_finish first"; return SSG_EINVAL; }
	ssg_recs *const r = m->r;
	if (r->ordered) { ssg_err_msg = who + ": refused while an order is declared: ssg_recs_reopen first"; return SSG_EINVAL; }
	const bool arrays = loc && ent, counting = cap == 0 && !loc && !ent;
	if (!arrays && !counting) { ssg_err_msg = who + ": no loc[] / ent[] (both NULL and cap == 0 is the counting form)"; return SSG_EINVAL; }
	recs_scan_dev_t s;
	CHK(recs_scan_dev(r, "ssg_markdup_apply", chunk_id, hint, n_hints, first, ~(uint64_t)0, true, n_rec, s));
	const uint64_t n = *n_rec;
	if (n > m->n - m->a_ord) {
		ssg_err_msg = who + ": the chunk's " + std::to_string(n) + " records behind ordinal " + std::to_string(m->a_ord) + " run past the " + std::to_string(m->n) + " records of the first pass";
		return SSG_EINVAL;
	}
	if (n == 0) return 0;
	const uint64_t grid = (n + 255) / 256;   /* (below 2^31: the scan has checked it) */
	dbuf<uint32_t> d_cnt((size_t)grid + 1); dbuf<uint64_t> d_base((size_t)grid + 1); dbuf<unsigned long long> d_bad(1);
	if (!d_cnt.ok() || !d_base.ok() || !d_bad.ok()) { ssg_err_msg = "device allocation failed: the counts of ssg_markdup_apply"; return SSG_ENOMEM; }
	CHK(rt_memset(d_cnt.p + grid, 0, 4)); CHK(rt_memset(d_bad.p, 0xff, 8));
	uint8_t *const d_chunk = r->d_chunk[chunk_id];
	SSG_LAUNCH(ssg_k_md_apply, grid, 256, 0, d_chunk, (const uint64_t*)s.loc.p, (const ssg_bam_ent_t*)s.ent.p, (int64_t)n, (const md_ent_t*)m->ents.p, (const uint32_t*)m->d_bitmap, m->a_ord, (int32_t)(remove ? 1 : 0),
	           d_cnt.p, d_bad.p, (const uint64_t*)0, (uint64_t)0, (uint64_t*)0, (ssg_bam_ent_t*)0);
	CHK((prim_exsum<uint32_t, uint64_t>(d_cnt.p, d_base.p, (int64_t)grid + 1)));
	CHK(rt_sync());
	unsigned long long bad = 0; CHK(d_bad.down(&bad, 1));
	if (bad != ~0ull) { ssg_err_msg = who + ": the stream changed between the passes: the record of ordinal " + std::to_string(bad) + " has another block_size or name than in the first pass"; return SSG_EIO; }
	uint64_t k = 0; CHK(rt_d2h(&k, d_base.p + grid, 8));
	*n_kept = k;
	if (counting) return 0;
	if (k > cap) { ssg_err_msg = who + ": " + std::to_string(k) + " records kept, room for " + std::to_string(cap); return SSG_EOVERFLOW; }
	dbuf<uint64_t> d_loc((size_t)k + 1); dbuf<ssg_bam_ent_t> d_ent((size_t)k + 1);
	if (!d_loc.ok() || !d_ent.ok()) { ssg_err_msg = "device allocation failed: the kept records of ssg_markdup_apply"; return SSG_ENOMEM; }
	SSG_LAUNCH(ssg_k_md_apply, grid, 256, 0, d_chunk, (const uint64_t*)s.loc.p, (const ssg_bam_ent_t*)s.ent.p, (int64_t)n, (const md_ent_t*)m->ents.p, (const uint32_t*)m->d_bitmap, m->a_ord, (int32_t)(remove ? 1 : 0),
	           d_cnt.p, d_bad.p, (const uint64_t*)d_base.p, k, d_loc.p, d_ent.p);
	CHK(rt_sync());
	CHK(d_loc.down(loc, (size_t)k)); CHK(d_ent.down(ent, (size_t)k));
	m->a_ord += n;
	return 0;
}

} /* extern "C" */
