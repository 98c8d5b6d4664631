/*
 * ssg_rec_gather.cpp -- the records of `sambamba sort`'s input kept in HBM in the chunks they arrived in, and the sorted stream gathered from them on the
 * device (k_rec_gather.h): ssg_recs_create / append / order / gather / reopen / release / free, and the launcher ssg_bgzf_compress_recs
 * (ssg_bgzf.cpp) puts in front of the deflate kernel.  A translation unit of its own: a kernel added to ssg_bgzf.cpp or ssg_bgzf_frame.cpp would be
 * compiled next to kernels whose machine code is pinned (tools/isa_pin.py).
 */
#include <algorithm>
#include <vector>
#include "ssg_rt.h"
#include "k_rec_gather.h"
#include "../../include/ssgpu.h"
#include "ssg_index_int.h"
#include "ssg_recs_int.h"

SSG_ABI_FP_DEFINE(rec_gather)

extern "C" {

int ssg_recs_create(uint64_t cap_bytes, ssg_recs_t **out)
{
	if (rt_device_count() < 1) { ssg_err_msg = "no HIP device visible: libssgpu has no CPU path"; return SSG_ENODEV; }
	if (!out) { ssg_err_msg = "ssg_recs_create: no place for the handle"; return SSG_EINVAL; }
	ssg_recs *r = new ssg_recs();
	r->dev = ssg_cur_dev; r->cap = cap_bytes;
	*out = r;
	return 0;
}

void ssg_recs_free(ssg_recs_t *r)
{
	if (!r) return;
	recs_drop_order(r);
	for (uint8_t *p : r->d_chunk) rt_free_raw(p);
	delete r;
}

int ssg_recs_append(ssg_recs_t *r, const uint8_t *bytes, uint64_t len, uint32_t *chunk_id)
{
	CHK(recs_usable(r, "ssg_recs_append"));
	if (r->ordered) { ssg_err_msg = "ssg_recs_append: the store is read-only once ssg_recs_order has declared the stream"; return SSG_EINVAL; }
	if (len > RG_OFF_MASK || r->d_chunk.size() >= ((size_t)1 << 24)) { ssg_err_msg = "ssg_recs_append: a chunk's offsets (40 bits) or the chunk ids (24 bits) do not fit a location"; return SSG_EINVAL; }
	if (len > r->cap || r->bytes > r->cap - len) { ssg_err_msg = "ssg_recs_append: the chunks would exceed the store's capacity"; return SSG_ENOMEM; }
	uint8_t *d = (uint8_t*)rt_malloc_raw((size_t)len + 16);
	if (!d) { ssg_err_msg = "device allocation failed: a chunk of records"; return SSG_ENOMEM; }
	const int rc = rt_h2d(d, bytes, (size_t)len);
	if (rc) { rt_free_raw(d); return rc; }
	if (chunk_id) *chunk_id = (uint32_t)r->d_chunk.size();
	r->d_chunk.push_back(d); r->len.push_back(len); r->bytes += len;
	return 0;
}

int ssg_recs_order(ssg_recs_t *r, const uint64_t *loc, const uint64_t *cum, int64_t n)
{
	CHK(recs_usable(r, "ssg_recs_order"));
	if (n < 0 || !cum || (n > 0 && !loc)) { ssg_err_msg = "ssg_recs_order: n < 0, or no loc[] / cum[]"; return SSG_EINVAL; }
	/* everything the kernel will load from is checked here: it has no bounds of its own */
	if (cum[0] != 0) { ssg_err_msg = "ssg_recs_order: cum[0] is not 0"; return SSG_EINVAL; }
	for (int64_t i = 0; i < n; ++i) {
		if (cum[i + 1] < cum[i]) { ssg_err_msg = "ssg_recs_order: cum[] decreases at record " + std::to_string(i); return SSG_EINVAL; }
		const uint64_t c = loc[i] >> 40, o = loc[i] & RG_OFF_MASK, l = cum[i + 1] - cum[i];
		if (c < r->d_chunk.size() && !r->d_chunk[(size_t)c]) { ssg_err_msg = "ssg_recs_order: record " + std::to_string(i) + " names chunk " + std::to_string(c) + ", which ssg_recs_release has released"; return SSG_EINVAL; }
		if (c >= r->d_chunk.size()) { ssg_err_msg = "ssg_recs_order: record " + std::to_string(i) + " names chunk " + std::to_string(c) + ", the store has " + std::to_string(r->d_chunk.size()); return SSG_EINVAL; }
		if (o > r->len[(size_t)c] || l > r->len[(size_t)c] - o) { ssg_err_msg = "ssg_recs_order: record " + std::to_string(i) + " runs past the end of chunk " + std::to_string(c); return SSG_EINVAL; }
	}
	recs_drop_order(r);
	const size_t nc = r->d_chunk.size();
	r->d_ptr = (uint8_t**)rt_malloc_raw(std::max<size_t>(nc, 1) * sizeof(uint8_t*));
	r->d_loc = (uint64_t*)rt_malloc_raw(std::max<size_t>((size_t)n, 1) * 8);
	r->d_cum = (uint64_t*)rt_malloc_raw(((size_t)n + 1) * 8);
	if (!r->d_ptr || !r->d_loc || !r->d_cum) { recs_drop_order(r); ssg_err_msg = "device allocation failed: the sorted order of the records"; return SSG_ENOMEM; }
	int rc = rt_h2d(r->d_ptr, r->d_chunk.data(), nc * sizeof(uint8_t*));
	if (!rc) rc = rt_h2d(r->d_loc, loc, (size_t)n * 8);
	if (!rc) rc = rt_h2d(r->d_cum, cum, ((size_t)n + 1) * 8);
	if (rc) { recs_drop_order(r); return rc; }
	r->n = n; r->total = cum[n]; r->ordered = true;
	return 0;
}

int ssg_recs_reopen(ssg_recs_t *r)
{
	CHK(recs_usable(r, "ssg_recs_reopen"));
	recs_drop_order(r);
	return 0;
}

int ssg_recs_release(ssg_recs_t *r, uint32_t chunk_id)
{
	CHK(recs_usable(r, "ssg_recs_release"));
	if (r->ordered) { ssg_err_msg = "ssg_recs_release: an order is declared (the gather may read the chunk): ssg_recs_reopen first"; return SSG_EINVAL; }
	if (chunk_id >= r->d_chunk.size() || !r->d_chunk[chunk_id]) { ssg_err_msg = "ssg_recs_release: chunk " + std::to_string(chunk_id) + " does not exist or is released already"; return SSG_EINVAL; }
	CHK(rt_sync());   /* (nothing queued on this thread's stream reads it any more) */
	rt_free_raw(r->d_chunk[chunk_id]);
	r->d_chunk[chunk_id] = 0; r->bytes -= r->len[chunk_id]; r->len[chunk_id] = 0;
	return 0;
}

/* stream bytes v0 .. v1 to d_out[0 .. v1 - v0) (room for that many bytes; a 256-byte aligned device buffer), queued on the calling thread's stream */
int ssg_recs_gather_dev(const ssg_recs_t *r, uint64_t v0, uint64_t v1, uint8_t *d_out)
{
	CHK(recs_usable(r, "ssg_recs_gather"));
	if (!r->ordered) { ssg_err_msg = "ssg_recs_gather: ssg_recs_order has not declared the stream"; return SSG_EINVAL; }
	if (v0 > v1 || v1 > r->total) { ssg_err_msg = "ssg_recs_gather: the range is not inside the stream (v0 <= v1 <= cum[n])"; return SSG_EINVAL; }
	if (v0 == v1) return 0;
	const uint64_t grid = (v1 - v0 + RG_TILE - 1) / RG_TILE;
	if (grid > 0x7fffffffu) { ssg_err_msg = "ssg_recs_gather: more than 2^31 tiles in one call"; return SSG_EINVAL; }
	SSG_LAUNCH(ssg_k_rec_gather, grid, 256, 0, (const uint8_t *const *)r->d_ptr, (const uint64_t*)r->d_loc, (const uint64_t*)r->d_cum, r->n, v0, v1, d_out);
	return 0;
}

int ssg_recs_gather(ssg_recs_t *r, uint64_t v0, uint64_t v1, uint8_t *out)
{
	CHK(recs_usable(r, "ssg_recs_gather"));
	if (!r->ordered) { ssg_err_msg = "ssg_recs_gather: ssg_recs_order has not declared the stream"; return SSG_EINVAL; }
	if (v0 > v1 || v1 > r->total) { ssg_err_msg = "ssg_recs_gather: the range is not inside the stream (v0 <= v1 <= cum[n])"; return SSG_EINVAL; }
	const uint64_t PIECE = (uint64_t)256 << 20;   /* per device call */
	dbuf<uint8_t> d_out((size_t)std::min(PIECE, v1 - v0) + 16);
	if (!d_out.ok()) { ssg_err_msg = "device allocation failed: gathered records"; return SSG_ENOMEM; }
	for (uint64_t a = v0; a < v1; a += PIECE) {
		const uint64_t b = std::min(v1, a + PIECE);
		CHK(ssg_recs_gather_dev(r, a, b, d_out.p));
		CHK(rt_sync());
		CHK(rt_d2h(out + (a - v0), d_out.p, (size_t)(b - a)));
	}
	return 0;
}

} /* extern "C" */
