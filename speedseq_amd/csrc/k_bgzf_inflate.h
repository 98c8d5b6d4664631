/*
 * k_bgzf_inflate.h -- RFC 1951 inflate of BGZF members on the device, the inverse of k_bgzf.h (the format's reader in the reference: htslib
 * bgzf.c, bgzf_read_block / inflate_block; the specification of the stream: RFC 1951 and zlib's inflate, whose verdict on a stream is this
 * kernel's).  A kernel of a translation unit of its own (ssg_bgzf_inflate.cpp): the machine code of the pinned kernels does not move.
 *
 * One wavefront per member, four per workgroup, a grid-stride loop over the members.  Per deflate block:
 *   1. lane 0 reads the block header; for a dynamic block the code lengths (into LDS), for both Huffman types the canonical code of each
 *      alphabet as zlib's puff does: count[len] and the symbols sorted by (length, symbol).  Every rule of zlib's inflate_table holds:
 *      over-subscribed sets fail, incomplete ones too unless the set is a single code of one bit, no end-of-block code fails, more than
 *      286 / 30 symbols fail.
 *   2. the wave fills the primary look-up tables in LDS (10 bits literal/length, 9 bits distance; entry = symbol << 4 | code length, 0 where
 *      the code is longer or does not exist): lane l walks the canonical code for entries l, l + 64, ...
 *   3. lane 0 decodes up to 64 symbols into LDS (literal, or length and distance); a code beyond the primary table walks the canonical code
 *      bit by bit.  It is the only lane that knows the bit position; it checks every symbol against what the member may still produce (ISIZE)
 *      and every distance against what has been produced, so that the placement below has nothing to check.
 *   4. the wave places the batch: wv_scan_add over the output lengths, all literals stored at once, then the matches in stream order, each
 *      copied by the whole wave, out[p + k] = out[p - dist + k % dist] (every source byte lies before p: no lane reads what the same match
 *      writes).  Stores read back by other lanes are fenced (ssg_wave_memsync): once behind the literals, and before a match whose source
 *      reaches into bytes stored since the last fence.
 *   A stored block is copied by the wave.  About 4.5 KB of LDS per wave; nothing of a member's output is kept in LDS.
 *
 * Safety, for arbitrary input bytes: the bit reader never fetches outside [in + s0, in + s1) (8-byte fetches only while 8 bytes remain, single
 * bytes behind that, zeros past the end -- and consuming a bit that was not there is an error); nothing is stored outside
 * out[o0 .. o0 + isize); every loop iteration consumes at least one bit or sets a flag that ends the loop; an error ends the member, the wave
 * goes on with its next one.  Loops leave by flags and one test.
 */
#ifndef SSG_K_BGZF_INFLATE_H
#define SSG_K_BGZF_INFLATE_H
#include "ssg_dev.h"

#define BZI_LBITS 10
#define BZI_DBITS 9
#define BZI_ST_OK 0
#define BZI_ST_MALFORMED 1
#define BZI_ST_LENGTH 2
/* flags of lane 0's decode steps */
#define BZI_F_ERR 1
#define BZI_F_OVER 2
#define BZI_F_EOB 4

struct bzi_lds_t {
	uint32_t sym[64], pos[64];                 /* a batch: literal 0x80000000 | byte, match length | (distance - 1) << 16; where each starts in the output */
	uint16_t ltab[1 << BZI_LBITS], dtab[1 << BZI_DBITS];
	uint16_t lsym[288], dsym[32], csym[20];    /* symbols sorted by (code length, symbol) */
	uint16_t lcnt[16], dcnt[16], ccnt[16], offs[16];
	uint8_t lens[320], cl[20];
};
struct bzi_rd_t { const uint8_t *in; uint32_t ip, iend; uint64_t bb; int bc; int err; };   /* bb: bc valid bits, the stream's next bit lowest */

static __device__ const uint8_t bzi_clorder[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };

/* at least 56 valid bits, or all that are left */
SSG_DEVFN void bzi_refill(bzi_rd_t &r)
{
	if (r.ip + 8u <= r.iend) {
		uint64_t w; __builtin_memcpy(&w, r.in + r.ip, 8);
		r.bb |= w << r.bc;                                     /* (bits above bc + 8 n are the stream's own: the next refill ORs the same ones in) */
		const int n = (63 - r.bc) >> 3;
		r.ip += (uint32_t)n; r.bc += n << 3;
	} else {
		int go = r.bc <= 56 && r.ip < r.iend;
		while (go) { r.bb |= (uint64_t)r.in[r.ip] << r.bc; ++r.ip; r.bc += 8; go = r.bc <= 56 && r.ip < r.iend; }
	}
}
SSG_DEVFN void bzi_drop(bzi_rd_t &r, int n)
{	/* n <= 48 */
	if (n > r.bc) { r.err = 1; n = r.bc; }
	r.bb >>= n; r.bc -= n;
}
SSG_DEVFN uint32_t bzi_bits(bzi_rd_t &r, int n) { const uint32_t v = (uint32_t)(r.bb & ((1ull << n) - 1ull)); bzi_drop(r, n); return v; }

/* the canonical code, bit by bit (puff.c's decode): the symbol of the code that starts at bit 0 of `b' and its length, among codes of at most
 * maxlen bits; -1 when there is none */
SSG_DEVFN int bzi_walk(uint64_t b, const uint16_t *cnt, const uint16_t *symt, int maxlen, int &len_out)
{
	int code = 0, first = 0, index = 0, s = -1;
	for (int len = 1; len <= maxlen; ++len) {
		code |= (int)(b & 1); b >>= 1;
		const int c = (int)cnt[len];
		if (s < 0 && code - c < first) { s = (int)symt[index + (code - first)]; len_out = len; }
		index += c; first += c; first <<= 1; code <<= 1;
	}
	return s;
}
/* one symbol: primary table, then the walk; consumes its bits.  No such code: r.err, one bit consumed */
SSG_DEVFN int bzi_symbol(bzi_rd_t &r, const uint16_t *tab, int pbits, const uint16_t *cnt, const uint16_t *symt)
{
	const uint32_t e = tab[r.bb & ((1u << pbits) - 1u)];
	int l = (int)(e & 15u), s = (int)(e >> 4);
	if (l == 0) {
		s = bzi_walk(r.bb, cnt, symt, 15, l);
		if (s < 0) { r.err = 1; s = 0; l = 1; }
	}
	bzi_drop(r, l);
	return s;
}
/* lane 0: count[], the sorted symbols; 0, or 1 when zlib's inflate_table would refuse the set (is_cl: the code-length code, which must be complete) */
SSG_DEVFN int bzi_canon(const uint8_t *lens, int n, uint16_t *cnt, uint16_t *offs, uint16_t *symt, int is_cl)
{
	for (int l = 0; l < 16; ++l) cnt[l] = 0;
	for (int s = 0; s < n; ++s) cnt[lens[s] & 15] = (uint16_t)(cnt[lens[s] & 15] + 1);
	cnt[0] = 0;
	int left = 1, bad = 0, max = 0;
	for (int l = 1; l < 16; ++l) { left <<= 1; left -= (int)cnt[l]; if (left < 0) { bad = 1; left = 0; } if (cnt[l]) max = l; }
	if (left > 0 && max != 0 && (is_cl || max != 1)) bad = 1;
	offs[1] = 0;
	for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + cnt[l]);
	for (int s = 0; s < n; ++s) { const int l = lens[s] & 15; if (l) { symt[offs[l]] = (uint16_t)s; offs[l] = (uint16_t)(offs[l] + 1); } }   /* (offs[l] < n: the counts add up to at most n) */
	return bad;
}
/* the wave: primary table of 1 << pbits entries */
SSG_DEVFN void bzi_fill(uint16_t *tab, int pbits, const uint16_t *cnt, const uint16_t *symt)
{
	for (int i = wv_lane(); i < (1 << pbits); i += SSG_WAVE) {
		int l = 0;
		const int s = bzi_walk((uint64_t)i, cnt, symt, pbits, l);
		tab[i] = s < 0 ? (uint16_t)0 : (uint16_t)(s << 4 | l);
	}
}
/* lane 0: a dynamic block's header behind its three type bits: L.lens[0 .. hlit + hdist) and both canonical codes; 0, or 1 for a malformed header */
SSG_DEVFN int bzi_dyn_header(bzi_rd_t &r, bzi_lds_t &L, int &hlit_out)
{
	bzi_refill(r);
	const int hlit = (int)bzi_bits(r, 5) + 257, hdist = (int)bzi_bits(r, 5) + 1, hclen = (int)bzi_bits(r, 4) + 4;
	int bad = hlit > 286 || hdist > 30;
	for (int i = 0; i < 19; ++i) L.cl[i] = 0;
	for (int i = 0; i < hclen; ++i) { if ((i & 7) == 0) bzi_refill(r); L.cl[bzi_clorder[i]] = (uint8_t)bzi_bits(r, 3); }
	bad |= bzi_canon(L.cl, 19, L.ccnt, L.offs, L.csym, 1);
	int any = 0; for (int l = 1; l < 8; ++l) any |= (int)L.ccnt[l];
	bad |= !any;                                                 /* no code at all: zlib reads zeros and then misses the end-of-block code */
	const int total = hlit + hdist;
	int i = 0;
	while (i < total && !bad && !r.err) {                        /* every turn consumes a bit or sets r.err */
		bzi_refill(r);
		int l = 1;
		const int s = bzi_walk(r.bb, L.ccnt, L.csym, 7, l);
		if (s < 0) bad = 1;
		else {
			bzi_drop(r, l);
			if (s < 16) { L.lens[i] = (uint8_t)s; ++i; }
			else {
				int rep, val = 0;
				if (s == 16) { rep = 3 + (int)bzi_bits(r, 2); if (i == 0) bad = 1; else val = L.lens[i - 1]; }
				else if (s == 17) rep = 3 + (int)bzi_bits(r, 3);
				else rep = 11 + (int)bzi_bits(r, 7);
				if (i + rep > total) bad = 1;
				else { for (int k = 0; k < rep; ++k) L.lens[i + k] = (uint8_t)val; i += rep; }
			}
		}
	}
	bad |= r.err;
	if (!bad) {
		if (L.lens[256] == 0) bad = 1;
		bad |= bzi_canon(L.lens, hlit, L.lcnt, L.offs, L.lsym, 0);
		bad |= bzi_canon(L.lens + hlit, hdist, L.dcnt, L.offs, L.dsym, 0);
	}
	hlit_out = hlit;
	return bad;
}

/* member b: the deflate stream in[rng[2b] .. rng[2b+1]) to out[ooff[b] .. ooff[b+1]); st[b]: 0, 1 (malformed), 2 (the stream's output is not ooff[b+1] - ooff[b] bytes).
 * The host has checked rng[2b] <= rng[2b+1] <= the bytes behind `in', and ooff[] against the bytes behind `out'. */
__global__ void __launch_bounds__(256) ssg_k_bgzf_inflate(const uint8_t *in, const uint64_t *rng, const uint64_t *ooff, long n_members, uint8_t *out, int32_t *st)
{
	__shared__ bzi_lds_t lds[4];
	bzi_lds_t &L = lds[(threadIdx.x >> 6) & 3];
	const int lane = wv_lane();
	const long wpb = (long)(blockDim.x >> 6);
	for (long b = (long)blockIdx.x * wpb + (long)(threadIdx.x >> 6); b < n_members; b += (long)gridDim.x * wpb) {
		const uint64_t s0 = rng[2 * b], s1 = rng[2 * b + 1];
		uint8_t *const o = out + ooff[b];
		const uint32_t isize = (uint32_t)(ooff[b + 1] - ooff[b]);
		bzi_rd_t r; r.in = in + s0; r.ip = 0; r.iend = (uint32_t)(s1 - s0); r.bb = 0; r.bc = 0; r.err = 0;
		uint32_t op = 0;                                           /* bytes produced: wave-uniform */
		int status = -1;                                           /* wave-uniform; -1: go on */
		ssg_wave_memsync();                                        /* (the previous member's LDS reads are done before lane 0 overwrites the tables) */
		while (status < 0) {                                       /* one deflate block a turn: at least its three header bits, or an error */
			/* ---- lane 0: the block's header ---- */
			int btype = 0, bfinal = 0, bad = 0, hlit = 288;
			uint32_t slen = 0, ssrc = 0;
			if (lane == 0) {
				bzi_refill(r);
				bfinal = (int)bzi_bits(r, 1); btype = (int)bzi_bits(r, 2);
				if (btype == 0) {
					/* back to a byte boundary: the whole bytes in the bit buffer return to the input */
					bzi_drop(r, r.bc & 7);
					r.ip -= (uint32_t)(r.bc >> 3); r.bb = 0; r.bc = 0;
					if (r.err || r.ip + 4u > r.iend) bad = 1;
					else {
						const uint32_t len = r.in[r.ip] | (uint32_t)r.in[r.ip + 1] << 8, nlen = r.in[r.ip + 2] | (uint32_t)r.in[r.ip + 3] << 8;
						r.ip += 4;
						if ((len ^ 0xffffu) != nlen || len > r.iend - r.ip) bad = 1;
						else { ssrc = r.ip; slen = len; r.ip += len; }
					}
				} else if (btype == 2) bad = bzi_dyn_header(r, L, hlit);
				else if (btype == 3) bad = 1;
				bad |= r.err;
			}
			btype = wv_get(btype, 0); bfinal = wv_get(bfinal, 0); bad = wv_get(bad, 0);
			int flags = bad ? BZI_F_ERR : 0;
			if (!flags && btype == 0) {
				/* ---- a stored block: the wave copies it ---- */
				slen = (uint32_t)wv_get((int)slen, 0); ssrc = (uint32_t)wv_get((int)ssrc, 0);
				if (slen > isize - op) flags = BZI_F_OVER;
				else {
					for (uint32_t k = (uint32_t)lane; k < slen; k += SSG_WAVE) o[op + k] = r.in[ssrc + k];
					op += slen;
					ssg_wave_memsync();
				}
			} else if (!flags) {
				/* ---- a Huffman block: the tables, then batches of symbols ---- */
				if (btype == 1) {
					for (int s = lane; s < 288; s += SSG_WAVE) L.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
					if (lane < 32) L.lens[288 + lane] = 5;
					ssg_wave_ldssync();
					if (lane == 0) { (void)bzi_canon(L.lens, 288, L.lcnt, L.offs, L.lsym, 0); (void)bzi_canon(L.lens + 288, 32, L.dcnt, L.offs, L.dsym, 0); }
				}
				ssg_wave_ldssync();
				bzi_fill(L.ltab, BZI_LBITS, L.lcnt, L.lsym);
				bzi_fill(L.dtab, BZI_DBITS, L.dcnt, L.dsym);
				ssg_wave_ldssync();
				while (!flags) {                                       /* one batch a turn: at least one bit, or a flag */
					int n = 0;
					if (lane == 0) {
						uint32_t made = op;
						while (n < 64 && !flags) {
							bzi_refill(r);
							const int s = bzi_symbol(r, L.ltab, BZI_LBITS, L.lcnt, L.lsym);
							if (r.err) flags = BZI_F_ERR;
							else if (s < 256) {
								if (made >= isize) flags = BZI_F_OVER;
								else { L.sym[n] = 0x80000000u | (uint32_t)s; ++n; ++made; }
							} else if (s == 256) flags = BZI_F_EOB;
							else if (s >= 286) flags = BZI_F_ERR;
							else {
								const int c = s - 257, leb = c < 8 || c == 28 ? 0 : (c >> 2) - 1;
								const uint32_t len = (c < 8 ? 3u + (uint32_t)c : c == 28 ? 258u : 3u + ((4u + (uint32_t)(c & 3)) << leb)) + bzi_bits(r, leb);
								const int d = bzi_symbol(r, L.dtab, BZI_DBITS, L.dcnt, L.dsym);
								const int deb = d < 4 ? 0 : (d >> 1) - 1;
								const uint32_t dist = (d < 4 ? 1u + (uint32_t)d : 1u + ((2u + (uint32_t)(d & 1)) << (deb & 15))) + bzi_bits(r, deb & 15);
								if (r.err || d >= 30 || dist > made) flags = BZI_F_ERR;
								else if (len > isize - made) flags = BZI_F_OVER;
								else { L.sym[n] = len | (dist - 1u) << 16; ++n; made += len; }
							}
						}
					}
					n = wv_get(n, 0); flags = wv_get(flags, 0);
					ssg_wave_ldssync();
					/* ---- the wave places the batch ---- */
					const uint32_t e = lane < n ? L.sym[lane] : 0u;
					const int is_lit = (int)(e >> 31), is_match = lane < n && !is_lit;
					const int olen = lane < n ? (is_lit ? 1 : (int)(e & 0xffffu)) : 0;
					const int incl = wv_scan_add(olen);
					const uint32_t p0 = op + (uint32_t)(incl - olen);
					if (lane < n && is_lit) o[p0] = (uint8_t)e;
					L.pos[lane] = p0;
					unsigned long long m = wv_ballot(is_match);
					ssg_wave_memsync();
					uint32_t dirty = 0xffffffffu;                          /* the lowest byte stored since the last fence */
					while (m) {
						const int j = __ffsll(m) - 1; m &= m - 1;
						const uint32_t ej = L.sym[j], p = L.pos[j], len = ej & 0xffffu, dist = (ej >> 16) + 1u;
						if (p - dist + (len < dist ? len : dist) > dirty) { ssg_wave_memsync(); dirty = 0xffffffffu; }
						for (uint32_t k = (uint32_t)lane; k < len; k += SSG_WAVE) o[p + k] = o[p - dist + (dist >= len ? k : k % dist)];
						dirty = dirty < p ? dirty : p;
					}
					op += (uint32_t)wv_get(incl, 63);
					ssg_wave_memsync();                                    /* the batch's stores before the next batch's loads; sym[] / pos[] read before lane 0 writes them again */
				}
			}
			if (flags & BZI_F_ERR) status = BZI_ST_MALFORMED;
			else if (flags & BZI_F_OVER) status = BZI_ST_LENGTH;
			else if (bfinal) status = op == isize ? BZI_ST_OK : BZI_ST_LENGTH;
		}
		if (lane == 0) st[b] = status;
	}
}
#endif
