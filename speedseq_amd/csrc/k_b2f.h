/*
 * k_b2f.h -- bamtofastq on the device: which two records of a BAM stream are a pair, in which order the pairs leave, and the FASTQ text itself (SURVEY.md
 * section 8 row f4; what the kernels stand for: main_tofastq and decode_read of host/bamkit_main.cpp, byte for byte).  The records lie in device memory: the
 * halves carried from earlier pushes (`carry', record c at cloc[c]) and behind them, in stream order, the records of a scanned chunk of the record store
 * (`chunk', loc[] as ssg_k_bam_walk left it).  Position p < n_carry is a carried record, p >= n_carry record p - n_carry of the chunk.  Kernels of a translation
 * unit of their own (ssg_b2f.cpp): the pinned machine code of the other kernels does not move.
 *
 *   ssg_k_b2f_facts, a lane per position: the malformed test (32 + l_qname + 4 n_cigar + (l_seq + 1) / 2 + l_seq > block_size; the smallest such offset goes to
 *     *bad), the walk of the CIGAR for a hard clip, the walk of the aux area with the host's type table (the last RG:Z before the walk ends), the -r list, a
 *     64-bit hash of the name masked to hash_bits.  Everything the later kernels read of a record -- name, sequence, qualities, the RG's span -- is seen to lie
 *     inside the record here: they have no bounds of their own.
 *   ssg_k_b2f_keys, a lane per eligible record: its hash, gathered for the sort.
 *   ssg_k_b2f_decide, a lane per eligible record in (hash, position) order: the lane at the start of a run of equal hashes walks the run in stream order with
 *     the host's state machine -- nothing held for the name: held; the held one has the same 0x40 bit: dropped; otherwise the pair is complete and nothing is
 *     held.  Names are compared in full, so two names with one hash are two machines inside one run and the result does not rest on the hash.  A run longer
 *     than SSG_B2F_RUN_MAX raises *flags bit 0 and decides nothing: no lane walks more than 256 records.  A sorted position outside [0, n) raises bit 1.
 *   ssg_k_b2f_marks, ssg_k_b2f_sizes, a lane per position: what the exclusive sums run over (completing records, held records and their bytes, a pair's text
 *     length -- with -n the width of counter + rank), and the compact lists of completing and held positions.
 *   ssg_k_b2f_text, a wave per half: lanes over the dwords of the output that the half touches.  A dword that lies wholly inside the half is stored as one; the
 *     up to three bytes at either end are byte stores (the neighbouring half writes the rest of that dword).  The 16 letters and their complements are four
 *     64-bit constants in registers.
 *   ssg_k_b2f_carry, a wave per held record: its bytes copied to the new carry.
 * Loops whose trip count differs per lane have no break / continue: they are left by their condition.
 */
#ifndef SSG_K_B2F_H
#define SSG_K_B2F_H
#include "ssg_dev.h"
#include "../../include/ssgpu.h"

#define B2F_OFF_MASK (((uint64_t)1 << 40) - 1)
#define B2F_ELIG 1u
#define B2F_FIRST 2u
#define B2F_REV 4u
/* state of a position: a partner's position (this record completes a pair with it), or one of */
#define B2F_NONE 0xffffffffu    /* not eligible */
#define B2F_HELD 0xfffffffeu
#define B2F_DROP 0xfffffffdu
#define B2F_TAKEN 0xfffffffcu   /* was held, left as the other half of a later record's pair */

struct b2f_fact_t { uint64_t hash; uint32_t rg_off, rg_len, nl, l_seq, flags, bs; };   /* rg_off: from the record's body; nl: the name's bytes; bs: block_size */

/* the block_size word of the record at position p */
SSG_DEVFN const uint8_t *b2f_rec(const uint8_t *carry, const uint64_t *cloc, uint32_t n_carry, const uint8_t *chunk, const uint64_t *loc, uint32_t p)
{
	return p < n_carry ? carry + cloc[p] : chunk + (loc[p - n_carry] & B2F_OFF_MASK);
}
SSG_DEVFN uint32_t b2f_ld32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
SSG_DEVFN bool b2f_same_bytes(const uint8_t *a, const uint8_t *b, uint32_t n)
{
	bool eq = true;
	for (uint32_t t = 0; t < n; ++t) eq = eq && a[t] == b[t];
	return eq;
}
SSG_DEVFN uint32_t b2f_digits(uint64_t v) { uint32_t d = 1; while (v >= 10) { v /= 10; ++d; } return d; }
/* the text of a half without its name: '@' '/' '1' [" RG:Z:" rg] '\n' seq "\n+\n" qual '\n' */
SSG_DEVFN uint64_t b2f_half_len(const b2f_fact_t &f) { return 8u + 2u * (uint64_t)f.l_seq + (f.rg_len ? 6u + (uint64_t)f.rg_len : 0u); }

__global__ void __launch_bounds__(256) ssg_k_b2f_facts(const uint8_t *carry, const uint64_t *cloc, uint32_t n_carry, const uint8_t *chunk, const uint64_t *loc, uint32_t n,
                                                       const uint8_t *rg_ids, const uint32_t *rg_off, int32_t n_rg, int32_t hash_bits,
                                                       b2f_fact_t *fact, uint8_t *elig, uint32_t *idx, unsigned long long *bad)
{
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p >= n) return;
	const uint8_t *rec = b2f_rec(carry, cloc, n_carry, chunk, loc, p), *body = rec + 4;
	uint32_t x[6]; memcpy(x, rec, 24);   /* block_size, tid, pos, bin_mq_nl, flag_nc, l_seq: the scan has seen that 4 + block_size >= 36 bytes lie inside */
	const uint32_t bs = x[0], lq = x[3] & 0xffu, nc = x[4] & 0xffffu, flag = x[4] >> 16, l = x[5];
	b2f_fact_t f; f.hash = 0; f.rg_off = f.rg_len = 0; f.nl = lq ? lq - 1u : 0u; f.l_seq = l; f.flags = 0; f.bs = bs;
	uint64_t a = 32u + (uint64_t)lq + 4u * (uint64_t)nc + ((uint64_t)l + 1u) / 2u + (uint64_t)l;
	const uint64_t e = bs;
	const bool good = a <= e;
	if (!good) { f.l_seq = 0; f.nl = 0; if (p >= n_carry) atomicMin(bad, (unsigned long long)(loc[p - n_carry] & B2F_OFF_MASK)); }
	bool hard = false;
	if (good) {
		const uint8_t *cig = body + 32 + lq;
		for (uint32_t k = 0; k < nc; ++k) hard = hard || (b2f_ld32(cig + 4 * (uint64_t)k) & 0xfu) == 5u;
	}
	/* the aux area, as decode_read walks it: an unknown type (`d' among them), a Z / H without its NUL and a B without its five bytes end the walk */
	bool go = good && a + 3 <= e;
	while (go) {
		const uint8_t t0 = body[a], t1 = body[a + 1], ty = body[a + 2];
		a += 3;
		uint64_t sz = 0; bool stop = false;
		if (ty == 'A' || ty == 'c' || ty == 'C') sz = 1;
		else if (ty == 's' || ty == 'S') sz = 2;
		else if (ty == 'i' || ty == 'I' || ty == 'f') sz = 4;
		else if (ty == 'Z' || ty == 'H') {
			uint64_t q = a;
			while (q < e && body[q] != 0) ++q;
			stop = q >= e;
			if (!stop && t0 == 'R' && t1 == 'G' && ty == 'Z') { f.rg_off = (uint32_t)a; f.rg_len = (uint32_t)(q - a); }
			sz = q - a + 1;
		} else if (ty == 'B') {
			stop = a + 5 > e;
			if (!stop) {
				const uint8_t st = body[a]; const uint64_t cnt = b2f_ld32(body + a + 1);
				sz = 5 + ((st == 'c' || st == 'C') ? 1u : (st == 's' || st == 'S') ? 2u : 4u) * cnt;
			}
		} else stop = true;
		a += sz;
		go = !stop && a + 3 <= e;
	}
	bool want = n_rg == 0;
	for (int32_t g = 0; g < n_rg; ++g) {
		const uint32_t o = rg_off[g], gl = rg_off[g + 1] - o;
		if (gl == f.rg_len && b2f_same_bytes(rg_ids + o, body + f.rg_off, gl)) want = true;
	}
	uint64_t h = 0xcbf29ce484222325ull;   /* FNV-1a over the name, then a finishing mix: the low bits are what a narrow hash_bits keeps */
	for (uint32_t t = 0; t < f.nl; ++t) { h ^= body[32 + t]; h *= 0x100000001b3ull; }
	h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
	f.hash = hash_bits >= 64 ? h : hash_bits <= 0 ? 0 : h & (((uint64_t)1 << hash_bits) - 1);
	const bool el = good && !(flag & 0x900u) && (flag & 1u) && !hard && want;
	f.flags = (el ? B2F_ELIG : 0u) | (flag & 0x40u ? B2F_FIRST : 0u) | (flag & 0x10u ? B2F_REV : 0u);
	fact[p] = f; elig[p] = el ? 1 : 0; idx[p] = p;
}

__global__ void __launch_bounds__(256) ssg_k_b2f_keys(const b2f_fact_t *fact, const uint32_t *epos, uint32_t m, uint32_t n, uint64_t *key)
{
	const uint32_t j = blockIdx.x * 256u + threadIdx.x;
	if (j >= m) return;
	const uint32_t p = epos[j];
	key[j] = p < n ? fact[p].hash : 0;
}

__global__ void __launch_bounds__(256) ssg_k_b2f_decide(const uint8_t *carry, const uint64_t *cloc, uint32_t n_carry, const uint8_t *chunk, const uint64_t *loc, uint32_t n,
                                                        const b2f_fact_t *fact, const uint64_t *key, const uint32_t *pos, uint32_t m, uint32_t *state, uint32_t *flags)
{
	const uint32_t j = blockIdx.x * 256u + threadIdx.x;
	if (j >= m) return;
	const uint64_t k0 = key[j];
	if (pos[j] >= n) { atomicOr(flags, 2u); return; }
	if (j > 0 && key[j - 1] == k0) return;   /* not the start of a run */
	uint32_t len = 1; bool sane = true;
	while (len <= SSG_B2F_RUN_MAX && j + len < m && key[j + len] == k0) { sane = sane && pos[j + len] < n; ++len; }
	if (len > SSG_B2F_RUN_MAX) { atomicOr(flags, 1u); return; }
	if (!sane) { atomicOr(flags, 2u); return; }
	for (uint32_t i = 0; i < len; ++i) {
		const uint32_t p = pos[j + i];
		const uint32_t nl = fact[p].nl, first = fact[p].flags & B2F_FIRST;
		const uint8_t *name = b2f_rec(carry, cloc, n_carry, chunk, loc, p) + 36;
		uint32_t held = B2F_NONE;   /* the held record of this name: at most one */
		for (uint32_t k = 0; k < i; ++k) {
			const uint32_t q = pos[j + k];
			if (held == B2F_NONE && state[q] == B2F_HELD && fact[q].nl == nl && b2f_same_bytes(b2f_rec(carry, cloc, n_carry, chunk, loc, q) + 36, name, nl)) held = q;
		}
		if (held == B2F_NONE) state[p] = B2F_HELD;
		else if ((fact[held].flags & B2F_FIRST) == first) state[p] = B2F_DROP;
		else { state[p] = held; state[held] = B2F_TAKEN; }
	}
}

/* comp: 1 at a record that completes a pair; hbytes / hflag: the bytes of a held record and 1 */
__global__ void __launch_bounds__(256) ssg_k_b2f_marks(const b2f_fact_t *fact, const uint32_t *state, uint32_t n, uint32_t *comp, uint32_t *hbytes, uint32_t *hflag)
{
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p >= n) return;
	const uint32_t s = state[p];
	comp[p] = s < n ? 1u : 0u;
	hbytes[p] = s == B2F_HELD ? 4u + fact[p].bs : 0u;
	hflag[p] = s == B2F_HELD ? 1u : 0u;
}

__global__ void __launch_bounds__(256) ssg_k_b2f_sizes(const b2f_fact_t *fact, const uint32_t *state, uint32_t n, const uint64_t *rank, const uint64_t *hidx, const uint64_t *hoff,
                                                       int32_t rename, uint64_t counter, uint64_t *plen, uint32_t *cpos, uint64_t n_pairs, uint32_t *hpos, uint64_t *nloc, uint64_t n_held)
{
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p >= n) return;
	const uint32_t s = state[p];
	uint64_t pl = 0;
	if (s < n) {
		const uint32_t nl = rename ? b2f_digits(counter + rank[p]) : fact[p].nl;
		pl = 2u * nl + b2f_half_len(fact[p]) + b2f_half_len(fact[s]);
		if (rank[p] < n_pairs) cpos[rank[p]] = p;
	}
	plen[p] = pl;
	if (s == B2F_HELD && hidx[p] < n_held) { hpos[hidx[p]] = p; nloc[hidx[p]] = hoff[p]; }
}

/* byte k of a half's text; seq / qual: the record's packed bases and its qualities */
SSG_DEVFN uint32_t b2f_text_byte(uint64_t k, const uint8_t *name, uint32_t nl, int32_t rename, uint64_t number, uint32_t which, const uint8_t *rg, uint32_t rg_len,
                                 const uint8_t *seq, const uint8_t *qual, uint32_t l, bool rev, bool no_qual)
{
	const uint64_t LET_LO = 0x565352474d43413dull, LET_HI = 0x4e42444b48595754ull;   /* "=ACMGRSV" "TWYHKDBN", the first letter in the low byte */
	const uint64_t CMP_LO = 0x425359434b47543dull, CMP_HI = 0x4e56484d44525741ull;   /* "=TGKCYSB" "AWRDMHVN": A/T C/G M/K R/Y V/B H/D swapped */
	if (k == 0) return '@';
	k -= 1;
	if (k < nl) {
		if (!rename) return name[k];
		uint64_t v = number;
		for (uint32_t t = nl - 1 - (uint32_t)k; t > 0; --t) v /= 10;
		return '0' + (uint32_t)(v % 10);
	}
	k -= nl;
	if (k == 0) return '/';
	if (k == 1) return '1' + which;
	k -= 2;
	if (rg_len) {
		if (k < 6) return (uint32_t)(0x3a5a3a475220ull >> (8 * k)) & 0xffu;   /* " RG:Z:" */
		k -= 6;
		if (k < rg_len) return rg[k];
		k -= rg_len;
	}
	if (k == 0) return '\n';
	k -= 1;
	if (k < l) {
		const uint32_t i = rev ? l - 1 - (uint32_t)k : (uint32_t)k;
		const uint32_t c = (seq[i >> 1] >> ((~i & 1u) << 2)) & 15u;
		const uint64_t w = rev ? (c < 8 ? CMP_LO : CMP_HI) : (c < 8 ? LET_LO : LET_HI);
		return (uint32_t)(w >> (8 * (c & 7u))) & 0xffu;
	}
	k -= l;
	if (k < 3) return k == 1 ? '+' : '\n';
	k -= 3;
	if (k < l) return no_qual ? 'I' : ((uint32_t)qual[rev ? l - 1 - k : k] + 33u) & 0xffu;
	return '\n';
}

__global__ void __launch_bounds__(256) ssg_k_b2f_text(const uint8_t *carry, const uint64_t *cloc, uint32_t n_carry, const uint8_t *chunk, const uint64_t *loc, uint32_t n,
                                                      const b2f_fact_t *fact, const uint32_t *state, const uint32_t *cpos, const uint64_t *rank, const uint64_t *off, uint64_t n_pairs,
                                                      int32_t rename, uint64_t counter, uint8_t *out, uint64_t out_len)
{
	const uint64_t h = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
	if (h >= 2 * n_pairs) return;
	const uint32_t which = (uint32_t)(h & 1u);
	const uint32_t p = cpos[h >> 1];
	if (p >= n) return;
	const uint32_t q = state[p];
	if (q >= n) return;
	const uint32_t a = (fact[p].flags & B2F_FIRST) ? p : q, b = (fact[p].flags & B2F_FIRST) ? q : p;   /* the half with 0x40 is /1 */
	const uint64_t number = counter + rank[p];
	const uint32_t nl = rename ? b2f_digits(number) : fact[p].nl;
	const b2f_fact_t f = fact[which ? b : a];
	const uint64_t dest = off[p] + (which ? (uint64_t)nl + b2f_half_len(fact[a]) : 0u), end = dest + nl + b2f_half_len(f);
	const uint8_t *body = b2f_rec(carry, cloc, n_carry, chunk, loc, which ? b : a) + 4;
	const uint32_t lq = body[8], nc = b2f_ld32(body + 12) & 0xffffu, l = f.l_seq;
	const uint8_t *name = body + 32, *seq = body + 32 + lq + 4 * (uint64_t)nc, *qual = seq + (l + 1u) / 2u, *rg = body + f.rg_off;
	const bool rev = (f.flags & B2F_REV) != 0, no_qual = l > 0 && qual[0] == 0xff;
	for (uint64_t w = (dest >> 2) + (uint64_t)wv_lane(); 4 * w < end; w += 64) {
		const uint64_t o = 4 * w;
		uint32_t v = 0;
		SSG_UNROLL
		for (uint32_t t = 0; t < 4; ++t) {
			const uint64_t at = o + t;
			if (at >= dest && at < end) v |= b2f_text_byte(at - dest, name, nl, rename, number, which, rg, f.rg_len, seq, qual, l, rev, no_qual) << (8 * t);
		}
		if (o >= dest && o + 4 <= end && o + 4 <= out_len) memcpy(out + o, &v, 4);
		else {
			SSG_UNROLL
			for (uint32_t t = 0; t < 4; ++t) if (o + t >= dest && o + t < end && o + t < out_len) out[o + t] = (uint8_t)(v >> (8 * t));
		}
	}
}

__global__ void __launch_bounds__(256) ssg_k_b2f_carry(const uint8_t *carry, const uint64_t *cloc, uint32_t n_carry, const uint8_t *chunk, const uint64_t *loc, uint32_t n,
                                                       const b2f_fact_t *fact, const uint32_t *hpos, const uint64_t *nloc, uint64_t n_held, uint8_t *out, uint64_t out_len)
{
	const uint64_t h = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
	if (h >= n_held) return;
	const uint32_t p = hpos[h];
	if (p >= n) return;
	const uint8_t *rec = b2f_rec(carry, cloc, n_carry, chunk, loc, p);
	const uint64_t len = 4u + (uint64_t)fact[p].bs, o = nloc[h];
	for (uint64_t t = (uint64_t)wv_lane(); t < len; t += 64) if (o + t < out_len) out[o + t] = rec[t];
}
#endif
