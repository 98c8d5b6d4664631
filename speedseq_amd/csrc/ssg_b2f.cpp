/*
 * ssg_b2f.cpp -- ssg_b2f_create / push / waiting / free: bamtofastq on records that lie in the record store (k_b2f.h; the host
 * path it restates: main_tofastq, host/bamkit_main.cpp).  A push scans a chunk with the scan's own host code (recs_scan_dev, ssg_bam_scan.cpp), decides
 * eligibility, pairing and order on the device, writes the FASTQ text of the pairs the chunk's records complete there, and leaves the halves still held in a
 * device buffer of the object's own that counts against the store's capacity (the carry).  Nothing of the object, the store or the chunk changes before the
 * text has reached the caller: every array of a push is a temporary until then.  A translation unit of its own: the machine code of the pinned kernels does
 * not move (tools/isa_pin.py).
 */
#include <string>
#include <vector>
#include "ssg_rt.h"
#include "k_b2f.h"
#include "ssg_prim.h"
#include "../../include/ssgpu.h"
#include "ssg_recs_int.h"

struct ssg_b2f {
	ssg_recs *r; int rename, hash_bits; int32_t n_rg;
	uint8_t *d_ids; uint32_t *d_idoff;        /* the -r list: the ids' bytes one behind the other, n_rg + 1 offsets */
	uint8_t *d_carry; uint64_t *d_cloc;       /* the held halves' records in stream order, and where each begins */
	uint64_t n_carry, carry_bytes, counter;
	ssg_b2f() : r(0), rename(0), hash_bits(64), n_rg(0), d_ids(0), d_idoff(0), d_carry(0), d_cloc(0), n_carry(0), carry_bytes(0), counter(0) {}
};

extern "C" {

int ssg_b2f_create(ssg_recs_t *r, const char *const *rg, int n_rg, int rename, int hash_bits, ssg_b2f_t **out)
{
	if (!r) { ssg_err_msg = "ssg_b2f_create: no record store"; return SSG_EINVAL; }
	CHK(recs_usable(r, "ssg_b2f_create"));
	if (!out) { ssg_err_msg = "ssg_b2f_create: no place for the handle"; return SSG_EINVAL; }
	if (n_rg < 0 || (n_rg > 0 && !rg)) { ssg_err_msg = "ssg_b2f_create: n_rg < 0, or no rg[]"; return SSG_EINVAL; }
	if (hash_bits < 0 || hash_bits > 64) { ssg_err_msg = "ssg_b2f_create: hash_bits outside 0 .. 64"; return SSG_EINVAL; }
	std::vector<uint8_t> ids; std::vector<uint32_t> off(1, 0);
	for (int g = 0; g < n_rg; ++g) {
		if (!rg[g] || !rg[g][0]) { ssg_err_msg = "ssg_b2f_create: read group id " + std::to_string(g) + " is NULL or empty"; return SSG_EINVAL; }
		ids.insert(ids.end(), (const uint8_t*)rg[g], (const uint8_t*)rg[g] + strlen(rg[g]));
		if (ids.size() > 0x7fffffffu) { ssg_err_msg = "ssg_b2f_create: the read group ids exceed 2^31 bytes"; return SSG_EINVAL; }
		off.push_back((uint32_t)ids.size());
	}
	ssg_b2f *b = new ssg_b2f();
	b->r = r; b->rename = rename ? 1 : 0; b->hash_bits = hash_bits; b->n_rg = n_rg;
	b->d_ids = (uint8_t*)rt_malloc_raw(ids.size() + 16); b->d_idoff = (uint32_t*)rt_malloc_raw(off.size() * 4);
	int rc = b->d_ids && b->d_idoff ? 0 : SSG_ENOMEM;
	if (rc) ssg_err_msg = "device allocation failed: the read group ids of ssg_b2f_create";
	if (!rc) rc = rt_h2d(b->d_ids, ids.data(), ids.size());
	if (!rc) rc = rt_h2d(b->d_idoff, off.data(), off.size() * 4);
	if (rc) { rt_free_raw(b->d_ids); rt_free_raw(b->d_idoff); delete b; return rc; }
	*out = b;
	return 0;
}

void ssg_b2f_free(ssg_b2f_t *b)
{
	if (!b) return;
	(void)rt_sync();
	b->r->bytes -= b->carry_bytes;
	rt_free_raw(b->d_ids); rt_free_raw(b->d_idoff); rt_free_raw(b->d_carry); rt_free_raw(b->d_cloc);
	delete b;
}

int ssg_b2f_waiting(ssg_b2f_t *b, uint64_t *n_halves, uint64_t *bytes)
{
	if (!b) { ssg_err_msg = "ssg_b2f_waiting: no object"; return SSG_EINVAL; }
	if (n_halves) *n_halves = b->n_carry;
	if (bytes) *bytes = b->carry_bytes;
	return 0;
}

int ssg_b2f_push(ssg_b2f_t *b, uint32_t chunk_id, const uint64_t *hint, int64_t n_hints, uint64_t first, uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint64_t *n_rec, uint64_t *n_pairs)
{
	const std::string who = "ssg_b2f_push";
	if (!b) { ssg_err_msg = who + ": no object"; return SSG_EINVAL; }
	ssg_recs *const r = b->r;
	CHK(recs_usable(r, "ssg_b2f_push"));
	if (!out_len || !n_rec || !n_pairs) { ssg_err_msg = who + ": no place for the text's length, the number of records or the number of pairs"; return SSG_EINVAL; }
	*out_len = *n_rec = *n_pairs = 0;
	if (!out && out_cap) { ssg_err_msg = who + ": no out[]"; return SSG_EINVAL; }
	if (r->ordered) { ssg_err_msg = who + ": refused while an order is declared: ssg_recs_reopen first"; return SSG_EINVAL; }
	recs_scan_dev_t s;
	CHK(recs_scan_dev(r, "ssg_b2f_push", chunk_id, hint, n_hints, first, ~(uint64_t)0, true, n_rec, s));
	const uint64_t nc = b->n_carry, n64 = nc + *n_rec;
	if (n64 >= 0x7fffffffu) { ssg_err_msg = who + ": more than 2^31 records with the carried halves in one call"; return SSG_EINVAL; }
	const uint32_t n = (uint32_t)n64;
	const uint8_t *const d_chunk = r->d_chunk[chunk_id];
	uint64_t tot[4] = { 0, 0, 0, 0 };   /* pairs, text bytes, held halves, their bytes */
	uint8_t *d_ncarry = 0; uint64_t *d_ncloc = 0;
	struct own_t { uint8_t *&a; uint64_t *&l; ~own_t() { rt_free_raw(a); rt_free_raw(l); } } own = { d_ncarry, d_ncloc };
	if (n > 0) {
		const uint32_t grid = (n + 255u) / 256u;
		dbuf<b2f_fact_t> d_fact(n); dbuf<uint8_t> d_elig(n); dbuf<uint32_t> d_idx(n), d_epos(n), d_state(n); dbuf<unsigned long long> d_bad(1); dbuf<uint32_t> d_flags(1);
		if (!d_fact.ok() || !d_elig.ok() || !d_idx.ok() || !d_epos.ok() || !d_state.ok() || !d_bad.ok() || !d_flags.ok()) { ssg_err_msg = "device allocation failed: the facts of ssg_b2f_push"; return SSG_ENOMEM; }
		CHK(rt_memset(d_bad.p, 0xff, 8)); CHK(rt_memset(d_flags.p, 0, 4)); CHK(rt_memset(d_state.p, 0xff, (size_t)n * 4));
		const uint8_t *const carry = b->d_carry; const uint64_t *const cloc = b->d_cloc, *const loc = s.loc.p;
		SSG_LAUNCH(ssg_k_b2f_facts, grid, 256, 0, carry, cloc, (uint32_t)nc, d_chunk, loc, n, (const uint8_t*)b->d_ids, (const uint32_t*)b->d_idoff, b->n_rg, (int32_t)b->hash_bits,
		           d_fact.p, d_elig.p, d_idx.p, d_bad.p);
		uint64_t m = 0;
		CHK(prim_select((const uint32_t*)d_idx.p, (const uint8_t*)d_elig.p, (int64_t)n, d_epos.p, &m));   /* (ends in a download: the facts kernel is done) */
		unsigned long long bad = 0; CHK(d_bad.down(&bad, 1));
		if (bad != ~0ull) { ssg_err_msg = who + ": malformed record at offset " + std::to_string(bad) + ": 32 + l_qname + 4 n_cigar + (l_seq + 1) / 2 + l_seq exceeds block_size"; return SSG_EIO; }
		if (m > n) { ssg_err_msg = who + ": the selection returned more records than it was given"; return SSG_EHIP; }
		if (m > 0) {
			const uint32_t mgrid = ((uint32_t)m + 255u) / 256u;
			dbuf<uint64_t> d_key((size_t)m), d_skey((size_t)m); dbuf<uint32_t> d_spos((size_t)m);
			if (!d_key.ok() || !d_skey.ok() || !d_spos.ok()) { ssg_err_msg = "device allocation failed: the keys of ssg_b2f_push"; return SSG_ENOMEM; }
			SSG_LAUNCH(ssg_k_b2f_keys, mgrid, 256, 0, (const b2f_fact_t*)d_fact.p, (const uint32_t*)d_epos.p, (uint32_t)m, n, d_key.p);
			CHK(prim_sort_pairs(d_key.p, d_skey.p, d_epos.p, d_spos.p, (int64_t)m, 0, 64));   /* stable: equal hashes stay in stream order */
			SSG_LAUNCH(ssg_k_b2f_decide, mgrid, 256, 0, carry, cloc, (uint32_t)nc, d_chunk, loc, n, (const b2f_fact_t*)d_fact.p, (const uint64_t*)d_skey.p, (const uint32_t*)d_spos.p, (uint32_t)m,
			           d_state.p, d_flags.p);
			CHK(rt_sync());
			uint32_t fl = 0; CHK(d_flags.down(&fl, 1));
			if (fl & 2u) { ssg_err_msg = who + ": the sort returned a position outside the records"; return SSG_EHIP; }
			if (fl & 1u) { ssg_err_msg = who + ": more than " + std::to_string(SSG_B2F_RUN_MAX) + " eligible records share one name hash of " + std::to_string(b->hash_bits) + " bits"; return SSG_ERANGE; }
		}
		dbuf<uint32_t> d_comp((size_t)n + 1), d_hbytes((size_t)n + 1), d_hflag((size_t)n + 1); dbuf<uint64_t> d_rank((size_t)n + 1), d_hoff((size_t)n + 1), d_hidx((size_t)n + 1), d_plen((size_t)n + 1), d_off((size_t)n + 1);
		if (!d_comp.ok() || !d_hbytes.ok() || !d_hflag.ok() || !d_rank.ok() || !d_hoff.ok() || !d_hidx.ok() || !d_plen.ok() || !d_off.ok()) { ssg_err_msg = "device allocation failed: the sums of ssg_b2f_push"; return SSG_ENOMEM; }
		CHK(rt_memset(d_comp.p + n, 0, 4)); CHK(rt_memset(d_hbytes.p + n, 0, 4)); CHK(rt_memset(d_hflag.p + n, 0, 4)); CHK(rt_memset(d_plen.p + n, 0, 8));   /* (one more: a sum's last value is the total) */
		SSG_LAUNCH(ssg_k_b2f_marks, grid, 256, 0, (const b2f_fact_t*)d_fact.p, (const uint32_t*)d_state.p, n, d_comp.p, d_hbytes.p, d_hflag.p);
		CHK((prim_exsum<uint32_t, uint64_t>(d_comp.p, d_rank.p, (int64_t)n + 1)));
		CHK((prim_exsum<uint32_t, uint64_t>(d_hbytes.p, d_hoff.p, (int64_t)n + 1)));
		CHK((prim_exsum<uint32_t, uint64_t>(d_hflag.p, d_hidx.p, (int64_t)n + 1)));
		CHK(rt_sync());
		CHK(rt_d2h(&tot[0], d_rank.p + n, 8)); CHK(rt_d2h(&tot[2], d_hidx.p + n, 8)); CHK(rt_d2h(&tot[3], d_hoff.p + n, 8));
		if (tot[0] > n || tot[2] > n) { ssg_err_msg = who + ": a sum exceeds the number of records"; return SSG_EHIP; }
		dbuf<uint32_t> d_cpos((size_t)tot[0] + 1), d_hpos((size_t)tot[2] + 1);
		d_ncarry = (uint8_t*)rt_malloc_raw((size_t)tot[3] + 16); d_ncloc = (uint64_t*)rt_malloc_raw(((size_t)tot[2] + 1) * 8);
		if (!d_cpos.ok() || !d_hpos.ok() || !d_ncarry || !d_ncloc) { ssg_err_msg = "device allocation failed: the carry of ssg_b2f_push"; return SSG_ENOMEM; }
		SSG_LAUNCH(ssg_k_b2f_sizes, grid, 256, 0, (const b2f_fact_t*)d_fact.p, (const uint32_t*)d_state.p, n, (const uint64_t*)d_rank.p, (const uint64_t*)d_hidx.p, (const uint64_t*)d_hoff.p,
		           (int32_t)b->rename, b->counter, d_plen.p, d_cpos.p, tot[0], d_hpos.p, d_ncloc, tot[2]);
		CHK((prim_exsum<uint64_t, uint64_t>(d_plen.p, d_off.p, (int64_t)n + 1)));
		CHK(rt_sync());
		CHK(rt_d2h(&tot[1], d_off.p + n, 8));
		*out_len = tot[1];
		if (tot[1] > out_cap) { ssg_err_msg = who + ": " + std::to_string(tot[1]) + " bytes of text, room for " + std::to_string(out_cap); return SSG_EOVERFLOW; }
		dbuf<uint8_t> d_out((size_t)tot[1] + 16);
		if (!d_out.ok()) { ssg_err_msg = "device allocation failed: the text of ssg_b2f_push"; return SSG_ENOMEM; }
		SSG_LAUNCH(ssg_k_b2f_text, (2 * tot[0] + 3) / 4, 256, 0, carry, cloc, (uint32_t)nc, d_chunk, loc, n, (const b2f_fact_t*)d_fact.p, (const uint32_t*)d_state.p, (const uint32_t*)d_cpos.p,
		           (const uint64_t*)d_rank.p, (const uint64_t*)d_off.p, tot[0], (int32_t)b->rename, b->counter, d_out.p, tot[1]);
		SSG_LAUNCH(ssg_k_b2f_carry, (tot[2] + 3) / 4, 256, 0, carry, cloc, (uint32_t)nc, d_chunk, loc, n, (const b2f_fact_t*)d_fact.p, (const uint32_t*)d_hpos.p, (const uint64_t*)d_ncloc, tot[2], d_ncarry, tot[3]);
		CHK(rt_sync());
		CHK(rt_d2h(out, d_out.p, (size_t)tot[1]));
	}
	/* the text is with the caller: the chunk goes, the carry becomes the halves still held */
	CHK(ssg_recs_release(r, chunk_id));
	if (n > 0) {
		rt_free_raw(b->d_carry); rt_free_raw(b->d_cloc);
		b->d_carry = d_ncarry; b->d_cloc = d_ncloc; d_ncarry = 0; d_ncloc = 0;
		r->bytes -= b->carry_bytes; r->bytes += tot[3];
		b->n_carry = tot[2]; b->carry_bytes = tot[3];
	}
	b->counter += tot[0];
	*n_pairs = tot[0];
	return 0;
}

} /* extern "C" */
