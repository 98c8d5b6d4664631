/*
 * k_bgzf_frame.h -- what turns the deflate streams of k_bgzf.h into complete BGZF members on the device (the
 * format's writer in the reference: htslib bgzf.c:298-342): the CRC-32 of every payload, and the framing
 *     1f 8b 08 04 | 00 00 00 00 | 00 ff | 06 00 | 42 43 02 00 | BSIZE (u16: member bytes - 1) | deflate stream | CRC32 (u32) | ISIZE (u32).
 * Kernels of a translation unit of their own (ssg_bgzf_frame.cpp): the machine code of ssg_k_bgzf_deflate / ssg_k_bgzf_compact does not move.
 *
 * CRC-32 (zlib's: reflected polynomial 0xedb88320, initial value and final xor 0xffffffff), one wave per byte range of any length:
 *   1. lane l takes the l-th contiguous stretch of the range (a multiple of 16 bytes long, so every lane's stretch has the alignment of the
 *      range's start; the last lanes' are shorter or empty) and runs the register of the table algorithm over it -- bytewise up to the first
 *      16-byte boundary, slice-by-4 on aligned 16-byte loads from there, bytewise for what is left.  Lane 0 starts from 0xffffffff, the
 *      others from 0: the register is linear in (initial value, message), so the conditioning belongs to the lane that holds the first byte.
 *   2. the register after A || B is  reg(A) * x^(8|B|) + reg_0(B)  mod P  (what zlib's crc32_combine computes): every lane multiplies its
 *      register by x^(8 * bytes behind its stretch) -- square-and-multiply over a table of x^(2^k), a 32-step carry-less multiply each -- and
 *      the wave XORs the 64 products.  One final xor per range.  An empty range: 0xffffffff * x^0 ^ 0xffffffff = 0.
 * The tables (4 x 256 words slice-by-4, 32 words of x^(2^k)) are computed by the compiler and copied to LDS by the workgroup (four waves, each
 * with ranges of its own).  A look-up is a 4-byte LDS read: the wave is served in two groups of 32 lanes, a word's bank is (address / 4) mod 32, so
 * each 1 KB table lies eight words deep on every bank and 32 lanes with random bytes meet a few ways of conflict per access (equal bytes --
 * runs -- broadcast).  The kernel reads every byte once; it is expected, not yet measured, to be a small fraction of the deflate kernel's time on
 * the same payload.  One wave works on a whole range: right for BGZF blocks, slow for a single very long range.
 */
#ifndef SSG_K_BGZF_FRAME_H
#define SSG_K_BGZF_FRAME_H
#include "ssg_dev.h"

#define BZF_POLY 0xedb88320u
/* a(x) * b(x) mod P, bit 31 = x^0 (zlib crc32.c multmodp) */
constexpr uint32_t bzf_mulmod_c(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	for (int i = 0; i < 32; ++i) { if (a & (0x80000000u >> i)) p ^= b; b = (b & 1u) ? (b >> 1) ^ BZF_POLY : b >> 1; }
	return p;
}
struct bzf_tabs_t { uint32_t t[4][256]; uint32_t x2n[32]; };
constexpr bzf_tabs_t bzf_make_tabs()
{
	bzf_tabs_t r = {};
	for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ BZF_POLY : c >> 1; r.t[0][i] = c; }
	for (int s = 1; s < 4; ++s) for (uint32_t i = 0; i < 256; ++i) r.t[s][i] = (r.t[s - 1][i] >> 8) ^ r.t[0][r.t[s - 1][i] & 0xff];   /* one more zero byte behind */
	uint32_t p = 0x40000000u;   /* x^1 */
	r.x2n[0] = p;
	for (int k = 1; k < 32; ++k) r.x2n[k] = p = bzf_mulmod_c(p, p);   /* x^(2^k); x^(2^32) = x: the table is cyclic */
	return r;
}
static __device__ const bzf_tabs_t bzf_tabs = bzf_make_tabs();
static_assert(bzf_make_tabs().t[0][1] == 0x77073096u && bzf_make_tabs().t[0][255] == 0x2d02ef8du, "CRC-32 byte table");
static_assert(bzf_make_tabs().x2n[3] == 0x00800000u, "x^8");

SSG_DEVFN uint32_t bzf_mulmod(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	SSG_UNROLL for (int i = 0; i < 32; ++i) { p ^= (a & (0x80000000u >> i)) ? b : 0u; b = (b >> 1) ^ ((b & 1u) ? BZF_POLY : 0u); }
	return p;
}
SSG_DEVFN uint32_t bzf_crc_byte(const uint32_t *tab, uint32_t c, uint32_t byte) { return tab[(c ^ byte) & 0xff] ^ (c >> 8); }
SSG_DEVFN uint32_t bzf_crc_word(const uint32_t *tab, uint32_t c, uint32_t w)
{	/* four bytes, the lowest first */
	c ^= w;
	return tab[768 + (c & 0xff)] ^ tab[512 + ((c >> 8) & 0xff)] ^ tab[256 + ((c >> 16) & 0xff)] ^ tab[c >> 24];
}

#ifndef SSG_BZF_TABLES_ONLY   /* (k_stats.h takes the tables and the two steps and leaves the kernels to their own translation unit) */
/* crc[i] = CRC-32 of data[cut[i] .. cut[i+1]), i < n_ranges; a wave takes ranges i, i + waves of the grid, ... */
__global__ void __launch_bounds__(256) ssg_k_crc32_ranges(const uint8_t *data, const uint64_t *cut, long n_ranges, uint32_t *crc)
{
	__shared__ uint32_t tab[4 * 256];
	__shared__ uint32_t x2n[32];
	for (int k = (int)threadIdx.x; k < 4 * 256; k += (int)blockDim.x) tab[k] = bzf_tabs.t[k >> 8][k & 255];
	if (threadIdx.x < 32) x2n[threadIdx.x] = bzf_tabs.x2n[threadIdx.x];
	__syncthreads();
	const int lane = wv_lane();
	const long wpb = (long)(blockDim.x >> 6);
	for (long i = (long)blockIdx.x * wpb + (long)(threadIdx.x >> 6); i < n_ranges; i += (long)gridDim.x * wpb) {
		const uint64_t s = cut[i], n = cut[i + 1] - s;
		const uint64_t per = ((n + 63) / 64 + 15) & ~(uint64_t)15;
		const uint64_t a0 = (uint64_t)lane * per < n ? (uint64_t)lane * per : n, a1 = a0 + per < n ? a0 + per : n;
		const uint8_t *p = data + s + a0, *const e = data + s + a1;
		uint32_t c = lane == 0 ? 0xffffffffu : 0u;
		while (p < e && ((uintptr_t)p & 15)) c = bzf_crc_byte(tab, c, *p++);
		for (; p + 16 <= e; p += 16) {
			const ssg_q16_t w = *(const ssg_q16_t*)p;
			c = bzf_crc_word(tab, c, w.v[0]); c = bzf_crc_word(tab, c, w.v[1]); c = bzf_crc_word(tab, c, w.v[2]); c = bzf_crc_word(tab, c, w.v[3]);
		}
		while (p < e) c = bzf_crc_byte(tab, c, *p++);
		/* c * x^(8 * bytes behind this lane's stretch): bit j of the byte count selects x^(2^(j+3)) */
		const uint64_t behind = n - a1;
		for (int j = 0; j < 64 && (n >> j) != 0; ++j) if ((behind >> j) & 1) c = bzf_mulmod(x2n[(j + 3) & 31], c);
		SSG_UNROLL for (int d = 1; d < 64; d <<= 1) c ^= (uint32_t)wv_shfl((int)c, lane ^ d);
		if (lane == 0) crc[i] = c ^ 0xffffffffu;
	}
}

/* Block b's member to dense[moff[b] .. moff[b+1]): the header, the stream the deflate kernel left at tmp + b * tmp_stride (moff[b+1] - moff[b] - 26
 * bytes of it), CRC-32 and ISIZE.  A block without payload becomes htslib's end-of-file marker -- the stream `03 00' (an empty block of the
 * fixed code), 28 bytes in all -- whatever the deflate kernel made of it: the host sizes such a member at 28. */
__global__ void __launch_bounds__(256) ssg_k_bgzf_frame(const uint8_t *tmp, uint32_t tmp_stride, const uint64_t *cut, const uint64_t *moff, const uint32_t *crc, int n_blocks, uint8_t *dense)
{
	const int b = (int)blockIdx.x, t = (int)threadIdx.x;
	if (b >= n_blocks) return;
	const uint32_t isize = (uint32_t)(cut[b + 1] - cut[b]), msize = (uint32_t)(moff[b + 1] - moff[b]), clen = msize - 26u;
	const uint8_t *s = tmp + (size_t)b * tmp_stride; uint8_t *d = dense + moff[b];
	if (t < 18) {
		const uint64_t h0 = 0x0000000004088b1full, h1 = 0x000243420006ff00ull;   /* the 16 fixed bytes, the lowest first */
		d[t] = t < 8 ? (uint8_t)(h0 >> (8 * t)) : t < 16 ? (uint8_t)(h1 >> (8 * (t - 8))) : (uint8_t)((msize - 1u) >> (8 * (t - 16)));
	}
	if (isize) { for (uint32_t k = (uint32_t)t; k < clen; k += blockDim.x) d[18 + k] = s[k]; }
	else if (t < 2) d[18 + t] = t ? 0 : 3;
	if (t >= 64 && t < 72) { const int j = t - 64; d[18 + clen + (uint32_t)j] = (uint8_t)((j < 4 ? crc[b] : isize) >> (8 * (j & 3))); }
}
#endif
#endif
