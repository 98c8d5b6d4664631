/*
 * ssg_bam_scan.cpp -- a BAM file read into the record store without its payload ever being in host memory (k_bam_scan.h; the
 * reader in the reference: bgzf_read_block and bam_read1, htslib): ssg_recs_append_bgzf inflates BGZF members into a new chunk of the store
 * (ssg_k_bgzf_inflate and the CRC-32 kernel through ssg_bgzf_inflate_dev, as they are), ssg_recs_scan finds the chunk's records and brings back the 40 bytes
 * of each that `sambamba merge' and `sambamba index' need.  A translation unit of its own: the machine code of the pinned kernels does not move
 * (tools/isa_pin.py).
 */
#include <algorithm>
#include <string>
#include <vector>
#include "ssg_rt.h"
#include "k_bam_scan.h"
#include "ssg_prim.h"
#include "../../include/ssgpu.h"
#include "ssg_index_int.h"
#include "ssg_recs_int.h"

static inline uint32_t ld_u32(const uint8_t *p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

/* the scan with its results left in device memory (ssg_recs_int.h): ssg_recs_scan copies them out, ssg_recs_select (ssg_bam_select.cpp) decides on them there */
int recs_scan_dev(ssg_recs *r, const char *who_, uint32_t chunk_id, const uint64_t *hint, int64_t n_hints, uint64_t first, uint64_t cap, bool arrays, uint64_t *n_rec, recs_scan_dev_t &o)
{
	const std::string who(who_);
	CHK(recs_usable(r, who_));
	if (!n_rec) { ssg_err_msg = who + ": no place for the number of records"; return SSG_EINVAL; }
	*n_rec = 0;
	if (chunk_id >= r->d_chunk.size() || !r->d_chunk[chunk_id]) { ssg_err_msg = who + ": chunk " + std::to_string(chunk_id) + " does not exist or is released"; return SSG_EINVAL; }
	if (n_hints < 0 || (n_hints > 0 && !hint)) { ssg_err_msg = who + ": n_hints < 0, or no hint[]"; return SSG_EINVAL; }
	if (n_hints == 0) return 0;
	/* everything the walk compares its offsets with is checked here */
	const uint64_t clen = r->len[chunk_id], total = hint[n_hints];
	for (int64_t b = 0; b < n_hints; ++b) if (hint[b + 1] < hint[b]) { ssg_err_msg = who + ": hint[] decreases at " + std::to_string(b); return SSG_EINVAL; }
	if (total > clen) { ssg_err_msg = who + ": hint[n_hints] lies behind the chunk's " + std::to_string(clen) + " bytes"; return SSG_EINVAL; }
	if (first > total) { ssg_err_msg = who + ": `first' lies behind hint[n_hints]"; return SSG_EINVAL; }
	const uint64_t grid = ((uint64_t)n_hints + 255) / 256;
	if (grid > 0x7fffffffu) { ssg_err_msg = who + ": more than 2^31 hints in one call"; return SSG_EINVAL; }
	const uint8_t *const d_chunk = r->d_chunk[chunk_id];
	const uint64_t tag = (uint64_t)chunk_id << 40;
	dbuf<uint64_t> d_hint((size_t)n_hints + 1), d_cnt((size_t)n_hints + 1), d_base((size_t)n_hints + 1), d_stop((size_t)n_hints);
	dbuf<uint32_t> d_state((size_t)n_hints);
	if (!d_hint.ok() || !d_cnt.ok() || !d_base.ok() || !d_stop.ok() || !d_state.ok()) { ssg_err_msg = "device allocation failed: the hints of a record scan"; return SSG_ENOMEM; }
	CHK(d_hint.up(hint, (size_t)n_hints + 1));
	CHK(rt_memset(d_cnt.p + n_hints, 0, 8));   /* (one count more: the scan's last value is the total) */
	SSG_LAUNCH(ssg_k_bam_walk, grid, 256, 0, d_chunk, total, (const uint64_t*)d_hint.p, n_hints, first, d_cnt.p, d_stop.p, d_state.p, (const uint64_t*)0, tag, (uint64_t)0, (uint64_t*)0);
	CHK((prim_exsum<uint64_t, uint64_t>(d_cnt.p, d_base.p, n_hints + 1)));
	CHK(rt_sync());
	std::vector<uint32_t> state((size_t)n_hints);
	CHK(d_state.down(state.data(), (size_t)n_hints));
	for (int64_t b = 0; b < n_hints; ++b) {
		if (state[(size_t)b] == BS_OK) continue;
		uint64_t stop = 0; CHK(rt_d2h(&stop, d_stop.p + b, 8));
		if (state[(size_t)b] == BS_SKEW) {
			ssg_err_msg = who + ": not record-aligned at hint " + std::to_string(b) + ": the walk that entered at offset " + std::to_string(std::max(hint[b], first)) + " passed hint " + std::to_string(b + 1) +
			              " (offset " + std::to_string(hint[b + 1]) + ") and stopped at offset " + std::to_string(stop) + ": no record begins there";
			return SSG_EALIGN;
		}
		ssg_err_msg = who + ": malformed record at offset " + std::to_string(stop) + (state[(size_t)b] == BS_SMALL ? ": a block_size below 32" : ": it runs past the end of the stream (offset " + std::to_string(total) + ")");
		return SSG_EIO;
	}
	uint64_t n = 0; CHK(rt_d2h(&n, d_base.p + n_hints, 8));
	*n_rec = n;
	if (n > cap) { ssg_err_msg = who + ": " + std::to_string(n) + " records, room for " + std::to_string(cap); return SSG_EOVERFLOW; }
	if (n == 0) return 0;
	if (!arrays) { ssg_err_msg = who + ": no loc[] / key[] / ent[]"; return SSG_EINVAL; }
	const uint64_t rgrid = (n + 255) / 256;
	if (rgrid > 0x7fffffffu) { ssg_err_msg = who + ": more than 2^39 records in one call"; return SSG_EINVAL; }
	dbuf<uint64_t> &d_loc = o.loc, &d_key = o.key; dbuf<ssg_bam_ent_t> &d_ent = o.ent; dbuf<unsigned long long> d_bad(1);
	if (!d_loc.alloc((size_t)n) || !d_key.alloc((size_t)n) || !d_ent.alloc((size_t)n) || !d_bad.ok()) { ssg_err_msg = "device allocation failed: the records of a scan"; return SSG_ENOMEM; }
	CHK(rt_memset(d_bad.p, 0xff, 8));
	SSG_LAUNCH(ssg_k_bam_walk, grid, 256, 0, d_chunk, total, (const uint64_t*)d_hint.p, n_hints, first, d_cnt.p, d_stop.p, d_state.p, (const uint64_t*)d_base.p, tag, n, d_loc.p);
	SSG_LAUNCH(ssg_k_bam_fields, rgrid, 256, 0, d_chunk, (const uint64_t*)d_loc.p, (int64_t)n, d_key.p, d_ent.p, d_bad.p);
	CHK(rt_sync());
	unsigned long long bad = 0; CHK(d_bad.down(&bad, 1));
	if (bad != ~0ull) { ssg_err_msg = who + ": malformed record at offset " + std::to_string(bad) + ": l_qname + 4 n_cigar exceeds block_size - 32"; return SSG_EIO; }
	return 0;
}

extern "C" {

int ssg_device_memory(uint64_t *free_bytes, uint64_t *total_bytes)
{
	if (rt_device_count() < 1) { ssg_err_msg = "no HIP device visible: libssgpu has no CPU path"; return SSG_ENODEV; }
#ifdef SSG_EMU
	const uint64_t f = (uint64_t)1 << 30, t = (uint64_t)1 << 30;   /* the emulation's "device" is host memory: a modest figure */
#else
	size_t f = 0, t = 0;
	CHK(rt_check(hipMemGetInfo(&f, &t), "hipMemGetInfo"));
#endif
	if (free_bytes) *free_bytes = (uint64_t)f;
	if (total_bytes) *total_bytes = (uint64_t)t;
	return 0;
}

int ssg_recs_append_bgzf(ssg_recs_t *r, const uint8_t *members, const uint64_t *moff, long n_blocks, uint32_t *chunk_id, uint64_t *out_off, int32_t *status)
{
	CHK(recs_usable(r, "ssg_recs_append_bgzf"));
	if (r->ordered) { ssg_err_msg = "ssg_recs_append_bgzf: the store is read-only once ssg_recs_order has declared the stream"; return SSG_EINVAL; }
	out_off[0] = 0;
	if (n_blocks <= 0) return 0;
	std::vector<uint64_t> rng((size_t)n_blocks * 2);
	CHK(ssg_bgzf_walk_members("ssg_recs_append_bgzf", members, moff, n_blocks, rng.data(), out_off));
	const uint64_t len = out_off[n_blocks];
	if (len > BS_OFF_MASK || r->d_chunk.size() >= ((size_t)1 << 24)) { ssg_err_msg = "ssg_recs_append_bgzf: a chunk's offsets (40 bits) or the chunk ids (24 bits) do not fit a location"; return SSG_EINVAL; }
	if (len > r->cap || r->bytes > r->cap - len) { ssg_err_msg = "ssg_recs_append_bgzf: the chunks would exceed the store's capacity"; return SSG_ENOMEM; }
	const long BB = 4096;   /* members per device call, as ssg_bgzf_inflate */
	const long nbmax = std::min(BB, n_blocks);
	uint64_t in_max = 0;
	for (long b0 = 0; b0 < n_blocks; b0 += BB) { const long nb = std::min(BB, n_blocks - b0); in_max = std::max(in_max, moff[b0 + nb] - moff[b0]); }
	dbuf<uint8_t> d_in((size_t)in_max + 16);
	dbuf<uint64_t> d_rng((size_t)nbmax * 2), d_ooff((size_t)nbmax + 1);
	dbuf<int32_t> d_st((size_t)nbmax); dbuf<uint32_t> d_crc((size_t)nbmax);
	if (!d_in.ok() || !d_rng.ok() || !d_ooff.ok() || !d_st.ok() || !d_crc.ok()) { ssg_err_msg = "device allocation failed: BGZF inflate"; return SSG_ENOMEM; }
	/* the chunk: owned by this call until every member has turned out good */
	struct own_t { uint8_t *p; ~own_t() { rt_free_raw(p); } } d = { (uint8_t*)rt_malloc_raw((size_t)len + 16) };
	if (!d.p) { ssg_err_msg = "device allocation failed: a chunk of records"; return SSG_ENOMEM; }
	std::vector<uint64_t> rel((size_t)nbmax * 2); std::vector<int32_t> st((size_t)nbmax); std::vector<uint32_t> crc((size_t)nbmax);
	long n_bad = 0, first_bad = -1;
	for (long b0 = 0; b0 < n_blocks; b0 += BB) {
		const long nb = std::min(BB, n_blocks - b0);
		const uint64_t ibase = moff[b0], ibytes = moff[b0 + nb] - ibase;
		for (long k = 0; k < 2 * nb; ++k) rel[(size_t)k] = rng[(size_t)(2 * b0 + k)] - ibase;
		/* (the output offsets as they are: every batch writes into the one chunk) */
		CHK(rt_h2d(d_in.p, members + ibase, ibytes)); CHK(d_rng.up(rel.data(), (size_t)nb * 2)); CHK(d_ooff.up(out_off + b0, (size_t)nb + 1));
		CHK(ssg_bgzf_inflate_dev(d_in.p, d_rng.p, d_ooff.p, nb, d.p, d_st.p, d_crc.p));
		CHK(rt_sync());
		CHK(d_st.down(st.data(), (size_t)nb)); CHK(d_crc.down(crc.data(), (size_t)nb));
		for (long k = 0; k < nb; ++k) {
			int32_t s = st[(size_t)k];
			if (s == 0 && crc[(size_t)k] != ld_u32(members + moff[b0 + k + 1] - 8)) s = 3;
			if (status) status[b0 + k] = s;
			if (s) { if (!n_bad) first_bad = b0 + k; ++n_bad; }
		}
	}
	if (n_bad) {
		ssg_err_msg = "ssg_recs_append_bgzf: " + std::to_string(n_bad) + " bad member(s), the first: member " + std::to_string(first_bad) + "; no chunk was added";
		return SSG_EIO;
	}
	if (chunk_id) *chunk_id = (uint32_t)r->d_chunk.size();
	r->d_chunk.push_back(d.p); r->len.push_back(len); r->bytes += len;
	d.p = 0;
	return 0;
}

int ssg_recs_scan(ssg_recs_t *r, uint32_t chunk_id, const uint64_t *hint, int64_t n_hints, uint64_t first, uint64_t cap, uint64_t *n_rec, uint64_t *loc, uint64_t *key, ssg_bam_ent_t *ent)
{
	recs_scan_dev_t o;
	CHK(recs_scan_dev(r, "ssg_recs_scan", chunk_id, hint, n_hints, first, cap, loc && key && ent, n_rec, o));
	const size_t n = (size_t)*n_rec;
	if (n) { CHK(o.loc.down(loc, n)); CHK(o.key.down(key, n)); CHK(o.ent.down(ent, n)); }
	return 0;
}

} /* extern "C" */
