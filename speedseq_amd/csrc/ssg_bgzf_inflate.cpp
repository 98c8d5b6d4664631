/*
 * ssg_bgzf_inflate.cpp -- BGZF inflate on the device (k_bgzf_inflate.h; the format's reader in the reference: htslib
 * bgzf.c, bgzf_read_block / check_header / inflate_block): ssg_bgzf_inflate, the inverse of ssg_bgzf_compress.  The host walks the members' headers,
 * the kernel inflates a wave per member, the CRC-32 kernel of ssg_bgzf_frame.cpp reads the output while it is in HBM, the host compares with the
 * trailers.  A translation unit of its own: the machine code of the pinned kernels does not move (tools/isa_pin.py).
 */
#include <algorithm>
#include <string>
#include <vector>
#include "ssg_rt.h"
#include "k_bgzf_inflate.h"
#include "../../include/ssgpu.h"
#include "ssg_index_int.h"


static inline uint32_t ld_u32(const uint8_t *p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

extern "C" {

/* every header (bgzf.c check_header: a gzip member with FEXTRA and a BC subfield of two bytes), the stream's bounds, ISIZE: rng[2b], rng[2b + 1] = the deflate
 * stream of member b in members[], out_off[] = the prefix sum of the ISIZEs.  SSG_EINVAL with `who' and the member in ssg_last_error() */
int ssg_bgzf_walk_members(const char *who, const uint8_t *members, const uint64_t *moff, long n_blocks, uint64_t *rng, uint64_t *out_off)
{
	out_off[0] = 0;
	auto refuse = [&](long b, const char *why) { ssg_err_msg = std::string(who) + ": member " + std::to_string(b) + ": " + why; return SSG_EINVAL; };
	for (long b = 0; b < n_blocks; ++b) {
		if (moff[b + 1] < moff[b] || moff[b + 1] - moff[b] < 28) return refuse(b, "a span shorter than 28 bytes");
		const uint8_t *h = members + moff[b]; const uint64_t span = moff[b + 1] - moff[b];
		if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return refuse(b, "not a gzip member with FEXTRA");
		const uint64_t xlen = h[10] | (uint64_t)h[11] << 8;
		if (12 + xlen + 8 > span) return refuse(b, "the extra field runs past the member");
		uint64_t bsize = 0;
		for (uint64_t o = 12; o + 4 <= 12 + xlen; ) { const uint64_t sl = h[o + 2] | (uint64_t)h[o + 3] << 8; if (h[o] == 'B' && h[o + 1] == 'C' && sl == 2 && o + 6 <= 12 + xlen) bsize = (uint64_t)(h[o + 4] | (uint64_t)h[o + 5] << 8) + 1; o += 4 + sl; }
		if (!bsize) return refuse(b, "no BC subfield");
		if (bsize != span) return refuse(b, "BSIZE + 1 differs from the member's span");
		const uint32_t isize = ld_u32(h + span - 4);
		if (isize > 65536) return refuse(b, "ISIZE above 65536");
		rng[(size_t)b * 2] = moff[b] + 12 + xlen; rng[(size_t)b * 2 + 1] = moff[b + 1] - 8;
		out_off[b + 1] = out_off[b] + isize;
	}
	return 0;
}

/* nb members (at most 4096 a call, as ssg_bgzf_compress: at most 256 MB in, 256 MB out) inflated and checksummed, queued on the calling thread's stream; device
 * buffers: member k's stream d_in[d_rng[2k] .. d_rng[2k + 1]) to d_out[d_ooff[k] .. d_ooff[k + 1]), d_st[k] as the kernel leaves it, d_crc[k] the output's CRC-32 */
int ssg_bgzf_inflate_dev(const uint8_t *d_in, const uint64_t *d_rng, const uint64_t *d_ooff, long nb, uint8_t *d_out, int32_t *d_st, uint32_t *d_crc)
{
	const long grid = std::min<long>((nb + 3) / 4, 4096);   /* four waves per workgroup, a wave per member */
	SSG_LAUNCH(ssg_k_bgzf_inflate, grid, 256, 0, d_in, d_rng, d_ooff, nb, d_out, d_st);
	return ssg_crc32_ranges_dev(d_out, d_ooff, nb, d_crc);   /* the output is in HBM: its checksum is one more read of it */
}

int ssg_bgzf_inflate(const uint8_t *members, const uint64_t *moff, long n_blocks, uint8_t *out, uint64_t out_cap, uint64_t *out_off, int32_t *status)
{
	if (rt_device_count() < 1) { ssg_err_msg = "no HIP device visible: libssgpu has no CPU path"; return SSG_ENODEV; }
	out_off[0] = 0;
	if (n_blocks <= 0) return 0;
	std::vector<uint64_t> rng((size_t)n_blocks * 2);
	CHK(ssg_bgzf_walk_members("ssg_bgzf_inflate", members, moff, n_blocks, rng.data(), out_off));
	if (out_off[n_blocks] > out_cap) { ssg_err_msg = "ssg_bgzf_inflate: output buffer too small"; return SSG_EOVERFLOW; }
	const long BB = 4096;   /* members per device call, as ssg_bgzf_compress: at most 256 MB in, 256 MB out */
	const long nbmax = std::min(BB, n_blocks);
	uint64_t in_max = 0, out_max = 0;
	for (long b0 = 0; b0 < n_blocks; b0 += BB) { const long nb = std::min(BB, n_blocks - b0); in_max = std::max(in_max, moff[b0 + nb] - moff[b0]); out_max = std::max(out_max, out_off[b0 + nb] - out_off[b0]); }
	dbuf<uint8_t> d_in((size_t)in_max + 16), d_out((size_t)out_max + 16);
	dbuf<uint64_t> d_rng((size_t)nbmax * 2), d_ooff((size_t)nbmax + 1);
	dbuf<int32_t> d_st((size_t)nbmax); dbuf<uint32_t> d_crc((size_t)nbmax);
	if (!d_in.ok() || !d_out.ok() || !d_rng.ok() || !d_ooff.ok() || !d_st.ok() || !d_crc.ok()) { ssg_err_msg = "device allocation failed: BGZF inflate"; return SSG_ENOMEM; }
	std::vector<uint64_t> rel((size_t)nbmax * 2), orel((size_t)nbmax + 1); std::vector<int32_t> st((size_t)nbmax); std::vector<uint32_t> crc((size_t)nbmax);
	long n_bad = 0, first_bad = -1;
	for (long b0 = 0; b0 < n_blocks; b0 += BB) {
		const long nb = std::min(BB, n_blocks - b0);
		const uint64_t ibase = moff[b0], ibytes = moff[b0 + nb] - ibase, obase = out_off[b0], obytes = out_off[b0 + nb] - obase;
		for (long k = 0; k < 2 * nb; ++k) rel[(size_t)k] = rng[(size_t)(2 * b0 + k)] - ibase;
		for (long k = 0; k <= nb; ++k) orel[(size_t)k] = out_off[b0 + k] - obase;
		CHK(rt_h2d(d_in.p, members + ibase, ibytes)); CHK(d_rng.up(rel.data(), (size_t)nb * 2)); CHK(d_ooff.up(orel.data(), (size_t)nb + 1));
		CHK(ssg_bgzf_inflate_dev(d_in.p, d_rng.p, d_ooff.p, nb, d_out.p, d_st.p, d_crc.p));
		CHK(rt_sync());
		CHK(d_st.down(st.data(), (size_t)nb)); CHK(d_crc.down(crc.data(), (size_t)nb));
		CHK(rt_d2h(out + obase, d_out.p, obytes));
		for (long k = 0; k < nb; ++k) {
			int32_t s = st[(size_t)k];
			if (s == 0 && crc[(size_t)k] != ld_u32(members + moff[b0 + k + 1] - 8)) s = 3;
			if (status) status[b0 + k] = s;
			if (s) { if (!n_bad) first_bad = b0 + k; ++n_bad; }
		}
	}
	if (n_bad) {
		ssg_err_msg = "ssg_bgzf_inflate: " + std::to_string(n_bad) + " bad member(s), the first: member " + std::to_string(first_bad);
		return SSG_EIO;
	}
	return 0;
}

} /* extern "C" */
