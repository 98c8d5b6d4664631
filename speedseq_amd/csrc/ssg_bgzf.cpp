/*
 * ssg_bgzf.cpp -- BGZF deflate on the device (k_bgzf.h): the host entry point of `sambamba sort`'s last
 * step.  A translation unit of its own (seconds to compile, variants by `make variant VUNITS=ssg_bgzf`).  ssg_bgzf_compress returns complete BGZF
 * members: the same deflate kernel, then the CRC-32 and framing kernels of ssg_bgzf_frame.cpp (k_bgzf_frame.h).  The *_level forms take the deflate level:
 * 1..6 are this unit's kernel (the bytes of the forms without a level), 7..9 the chained match finder of ssg_bgzf_deep.cpp (k_bgzf_deep.h) in its place.
 */
#include <algorithm>
#include <vector>
#include "ssg_rt.h"
#include "k_bgzf.h"
#include "../../include/ssgpu.h"
#include "ssg_index_int.h"

SSG_ABI_FP_DEFINE(bgzf)

extern "C" {

/* page-locked host memory from the library's pool (ssg_rt.h): copies to and from the device run at bus speed out of these */
void *ssg_host_alloc(size_t n) { return rt_host_alloc(n); }
void ssg_host_free(void *p) { rt_host_free(p); }

/* the blocks' deflate streams (frame = false: ssg_bgzf_deflate), or their complete members with the payloads' CRC-32 (frame = true: ssg_bgzf_compress) */
/* the payload: a host buffer, or (recs != NULL; ssg_bgzf_compress_recs) the sorted stream of a device-resident record store, cut[] in absolute stream offsets */
static int bgzf_run(const char *who, const uint8_t *payload, const ssg_recs_t *recs, const uint64_t *cut, long n_blocks, uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint32_t *crc, bool frame, int level)
{
	if (rt_device_count() < 1) { ssg_err_msg = "no HIP device visible: libssgpu has no CPU path"; return SSG_ENODEV; }
	if (level < 1 || level > 9) { ssg_err_msg = std::string(who) + ": the level must be 1..9 (the device writes no stored-only file; 1..6: one parse, 7..9: k_bgzf_deep.h)"; return SSG_EINVAL; }
	const int depth = ssg_bgzf_deep_depth(level);   /* 0: the shipped kernel */
	out_off[0] = 0;
	if (n_blocks <= 0) return 0;
	for (long b = 0; b < n_blocks; ++b) if (cut[b + 1] < cut[b] || cut[b + 1] - cut[b] > BZ_MAX_PAYLOAD) { ssg_err_msg = std::string(who) + ": a block's payload exceeds 0xff00 bytes"; return SSG_EINVAL; }
	const long BB = 4096;   /* blocks per device call: 256 MB of temporary output, 1 GB of symbol lists */
	const long nbmax = std::min(BB, n_blocks);
	dbuf<uint8_t> d_pay((size_t)nbmax * BZ_MAX_PAYLOAD + 16), d_tmp((size_t)nbmax * BZ_OUT_STRIDE), d_dense((size_t)nbmax * BZ_OUT_STRIDE);   /* (a member is at most 0xff00 + 5 + 26 bytes) */
	dbuf<uint32_t> d_sym((size_t)nbmax * BZ_STRETCH_CAP * 64), d_size(nbmax), d_crc(frame ? nbmax : 1);
	dbuf<uint64_t> d_cut(nbmax + 1), d_off(nbmax + 1);
	dbuf<uint16_t> d_prev(depth ? ssg_bgzf_deep_scratch(nbmax) / sizeof(uint16_t) : 1);   /* levels 7-9: the match finder's links of the earlier regions */
	if (!d_prev.ok()) { ssg_err_msg = "device allocation failed: BGZF deflate"; return SSG_ENOMEM; }
	if (!d_pay.ok() || !d_tmp.ok() || !d_dense.ok() || !d_sym.ok() || !d_size.ok() || !d_crc.ok() || !d_cut.ok() || !d_off.ok()) { ssg_err_msg = "device allocation failed: BGZF deflate"; return SSG_ENOMEM; }
	std::vector<uint64_t> rel((size_t)nbmax + 1), off((size_t)nbmax + 1); std::vector<uint32_t> sz((size_t)nbmax);
	for (long b0 = 0; b0 < n_blocks; b0 += BB) {
		const long nb = std::min(BB, n_blocks - b0);
		const uint64_t base = cut[b0], bytes = cut[b0 + nb] - base;
		for (long k = 0; k <= nb; ++k) rel[(size_t)k] = cut[b0 + k] - base;
		if (recs) CHK(ssg_recs_gather_dev(recs, base, base + bytes, d_pay.p));   /* (the gather kernel's last store may be a whole 16-byte granule: d_pay's slack) */
		else CHK(rt_h2d(d_pay.p, payload + base, bytes));
		CHK(d_cut.up(rel.data(), (size_t)nb + 1));
		if (depth) CHK(ssg_bgzf_deflate_deep_dev(d_pay.p, d_cut.p, nb, d_tmp.p, d_sym.p, d_size.p, d_prev.p, depth));
		else SSG_LAUNCH(ssg_k_bgzf_deflate, nb, 64, 0, (const uint8_t*)d_pay.p, (const uint64_t*)d_cut.p, (int)nb, d_tmp.p, d_sym.p, d_size.p);
		if (frame) CHK(ssg_crc32_ranges_dev(d_pay.p, d_cut.p, nb, d_crc.p));   /* the payload is in HBM for the deflate: its checksum is one more read of it */
		CHK(rt_sync());
		CHK(d_size.down(sz.data(), (size_t)nb));
		/* a member: 18 bytes of header, the stream, CRC-32 and ISIZE; without payload the 28-byte end-of-file marker (the stream `03 00', k_bgzf_frame.h) */
		off[0] = 0; for (long k = 0; k < nb; ++k) off[(size_t)k + 1] = off[(size_t)k] + (!frame ? sz[(size_t)k] : rel[(size_t)k + 1] == rel[(size_t)k] ? 28u : 26u + sz[(size_t)k]);
		if (out_off[b0] + off[(size_t)nb] > out_cap) { ssg_err_msg = std::string(who) + ": output buffer too small"; return SSG_EOVERFLOW; }
		CHK(d_off.up(off.data(), (size_t)nb + 1));
		if (frame) CHK(ssg_bgzf_frame_dev(d_tmp.p, BZ_OUT_STRIDE, d_cut.p, d_off.p, d_crc.p, nb, d_dense.p));
		else SSG_LAUNCH(ssg_k_bgzf_compact, nb, 256, 0, (const uint8_t*)d_tmp.p, (const uint64_t*)d_off.p, (int)nb, d_dense.p);
		CHK(rt_sync());
		CHK(rt_d2h(out + out_off[b0], d_dense.p, off[(size_t)nb]));
		if (frame && crc) CHK(d_crc.down(crc + b0, (size_t)nb));
		for (long k = 0; k < nb; ++k) out_off[b0 + k + 1] = out_off[b0] + off[(size_t)k + 1];
	}
	return 0;
}

int ssg_bgzf_deflate_level(const uint8_t *payload, const uint64_t *cut, long n_blocks, uint8_t *out, uint64_t out_cap, uint64_t *out_off, int level)
{
	return bgzf_run("ssg_bgzf_deflate_level", payload, 0, cut, n_blocks, out, out_cap, out_off, 0, false, level);
}
int ssg_bgzf_deflate(const uint8_t *payload, const uint64_t *cut, long n_blocks, uint8_t *out, uint64_t out_cap, uint64_t *out_off)
{
	return bgzf_run("ssg_bgzf_deflate", payload, 0, cut, n_blocks, out, out_cap, out_off, 0, false, 6);
}

int ssg_bgzf_compress_level(const uint8_t *payload, const uint64_t *cut, long n_blocks, uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint32_t *crc, int level)
{
	return bgzf_run("ssg_bgzf_compress_level", payload, 0, cut, n_blocks, out, out_cap, out_off, crc, true, level);
}
int ssg_bgzf_compress(const uint8_t *payload, const uint64_t *cut, long n_blocks, uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint32_t *crc)
{
	return bgzf_run("ssg_bgzf_compress", payload, 0, cut, n_blocks, out, out_cap, out_off, crc, true, 6);
}

int ssg_bgzf_compress_recs_level(ssg_recs_t *recs, const uint64_t *cut, long n_blocks, uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint32_t *crc, int level)
{
	if (!recs && rt_device_count() >= 1) { ssg_err_msg = "ssg_bgzf_compress_recs_level: no record store"; return SSG_EINVAL; }
	return bgzf_run("ssg_bgzf_compress_recs_level", 0, recs, cut, n_blocks, out, out_cap, out_off, crc, true, level);
}
int ssg_bgzf_compress_recs(ssg_recs_t *recs, const uint64_t *cut, long n_blocks, uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint32_t *crc)
{
	if (!recs && rt_device_count() >= 1) { ssg_err_msg = "ssg_bgzf_compress_recs: no record store"; return SSG_EINVAL; }
	return bgzf_run("ssg_bgzf_compress_recs", 0, recs, cut, n_blocks, out, out_cap, out_off, crc, true, 6);
}

} /* extern "C" */
