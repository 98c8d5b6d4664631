/*
 * ssg_bgzf_frame.cpp -- CRC-32 of byte ranges and BGZF framing on the device (k_bgzf_frame.h): ssg_crc32_batch,
 * ssg_bgzf_bound, and the two launchers ssg_bgzf_compress (ssg_bgzf.cpp) puts behind the deflate kernel.  A translation unit of its own: kernels added
 * to ssg_bgzf.cpp would be compiled next to ssg_k_bgzf_deflate, whose machine code is pinned (tools/isa_pin.py).
 */
#include <algorithm>
#include <vector>
#include "ssg_rt.h"
#include "k_bgzf_frame.h"
#include "../../include/ssgpu.h"
#include "ssg_index_int.h"

SSG_ABI_FP_DEFINE(bgzf_frame)

extern "C" {

/* queued on the calling thread's stream, behind what it has queued before; device buffers */
int ssg_crc32_ranges_dev(const uint8_t *d_data, const uint64_t *d_cut, long n, uint32_t *d_crc)
{
	const long grid = std::min<long>((n + 3) / 4, 4096);   /* four waves per workgroup, a wave per range */
	SSG_LAUNCH(ssg_k_crc32_ranges, grid, 256, 0, d_data, d_cut, n, d_crc);
	return 0;
}
int ssg_bgzf_frame_dev(const uint8_t *d_tmp, uint32_t tmp_stride, const uint64_t *d_cut, const uint64_t *d_moff, const uint32_t *d_crc, long n_blocks, uint8_t *d_dense)
{
	SSG_LAUNCH(ssg_k_bgzf_frame, n_blocks, 256, 0, d_tmp, tmp_stride, d_cut, d_moff, d_crc, (int)n_blocks, d_dense);
	return 0;
}

uint64_t ssg_bgzf_bound(uint64_t payload_bytes, long n_blocks) { return payload_bytes + 31 * (uint64_t)std::max(0l, n_blocks); }   /* stored form: 5; header and trailer: 26 */

int ssg_crc32_batch(const uint8_t *data, const uint64_t *cut, long n, uint32_t *crc)
{
	if (rt_device_count() < 1) { ssg_err_msg = "no HIP device visible: libssgpu has no CPU path"; return SSG_ENODEV; }
	if (n <= 0) return 0;
	for (long i = 0; i < n; ++i) if (cut[i + 1] < cut[i]) { ssg_err_msg = "ssg_crc32_batch: cut[] decreases"; return SSG_EINVAL; }
	const uint64_t BYTES = (uint64_t)256 << 20; const long RANGES = 1 << 20;   /* per device call: as many ranges as fit 256 MB (one range of any length does) */
	std::vector<uint64_t> rel;
	for (long i0 = 0; i0 < n; ) {
		long i1 = i0 + 1;
		while (i1 < n && i1 - i0 < RANGES && cut[i1 + 1] - cut[i0] <= BYTES) ++i1;
		const long m = i1 - i0; const uint64_t base = cut[i0], bytes = cut[i1] - base;
		dbuf<uint8_t> d_data((size_t)bytes + 16); dbuf<uint64_t> d_cut((size_t)m + 1); dbuf<uint32_t> d_crc((size_t)m);
		if (!d_data.ok() || !d_cut.ok() || !d_crc.ok()) { ssg_err_msg = "device allocation failed: CRC-32"; return SSG_ENOMEM; }
		rel.resize((size_t)m + 1);
		for (long k = 0; k <= m; ++k) rel[(size_t)k] = cut[i0 + k] - base;
		CHK(rt_h2d(d_data.p, data + base, bytes)); CHK(d_cut.up(rel.data(), (size_t)m + 1));
		CHK(ssg_crc32_ranges_dev(d_data.p, d_cut.p, m, d_crc.p));
		CHK(rt_sync());
		CHK(d_crc.down(crc + i0, (size_t)m));
		i0 = i1;
	}
	return 0;
}

} /* extern "C" */
