/*
 * k_markdup.h -- `sambamba markdup' on the device: Picard's duplicate rule over a stream of BAM records that passes twice (the rule: include/ssgpu.h, the
 * ssg_markdup_* comment).  The first pass leaves one entry per record in device memory, the decision runs over the entries alone, the second pass patches the
 * flag byte of the records and compacts the kept ones.  The records of a pass lie in a scanned chunk of the record store (`chunk', loc[] as ssg_k_bam_walk left
 * it).  Kernels of a translation unit of their own (ssg_markdup.cpp): the pinned machine code of the other kernels does not move.
 *
 *   ssg_k_md_ends, a lane per record: the malformed test (32 + l_qname + 4 n_cigar + (l_seq + 1) / 2 + l_seq > block_size; the smallest such offset goes to
 *     *bad), the taking-part and paired bits, the walk of the CIGAR for the unclipped 5' coordinate, the walk of the aux area with ssg_k_b2f_facts' type table
 *     (the last RG:Z before the walk ends) and the library of that value, a 64-bit hash of the name.  nlen[i]: the name's bytes when the record is paired (what
 *     the name arena takes of it), else 0.
 *   ssg_k_md_score, sixteen lanes per record: the qualities are read as aligned dwords, consecutive lanes consecutive dwords (64 bytes a step of the sixteen),
 *     the bytes outside the record's qualities masked away; every byte >= 15 is added, the sixteen sums meet by four butterfly steps, and lane 0 of the sixteen
 *     stores min(sum, 2^30 - 1).  The same lanes copy a paired record's name into the arena.  The chunk has 16 bytes of slack: an aligned dword that begins
 *     inside the chunk ends inside its allocation.
 *   ssg_k_md_bits: the OR of the u5, tid and library words of the taking-part entries: the radix sorts run over the bits in use only.
 *   ssg_k_md_pkeys, ssg_k_md_join: the mate join.  The paired entries sorted by (hash of hash_bits bits, ordinal); the lane at the start of a run of equal hashes
 *     walks the run in ordinal order -- nothing held for the name: held; the held one has the same flag & 0xc0: unmatched, the held one stays; otherwise the two
 *     are a pair and nothing is held.  Names are compared in full (the arena), so the result does not rest on the hash.  A run longer than SSG_MARKDUP_RUN_MAX
 *     raises *flags bit 0 and decides nothing: no lane walks more than 256 entries.
 *   ssg_k_md_pairs, ssg_k_md_frags: the elements of the two decisions as md_key_t: a pair's two end keys ordered by (tid, u5, rev, library), its score and its
 *     two ordinals; a taking-part record's end key, its score (a paired record: above every fragment's, and never marked) and its ordinal.
 *   ssg_k_md_word: one 64-bit word of the elements' keys in the current order, for a stable LSD radix pass (prim_sort_pairs).
 *   ssg_k_md_heads, ssg_k_md_pack, ssg_k_md_best, ssg_k_md_mark: the segmented arg-max.  head[i] = 1 where the sorted element i begins a group; behind an
 *     exclusive sum of the heads every element knows its group's number g, and (g, score, ~ordinal) is a 128-bit word whose inclusive running maximum
 *     (prim_scan_max), read at a group's last element, is the group's best: the highest score, the smallest ordinal among equals.  No lane walks a group: one
 *     of thousands of members costs what thousands of groups of one cost.  An element that is not its group's best sets the bits of its ordinals in the bitmap.
 *   ssg_k_md_apply, a lane per record of the second pass, run twice as ssg_k_bam_select is: the record's block_size and name hash against the entry of its
 *     ordinal (the smallest ordinal that differs goes to *bad), the kept lanes counted per workgroup; then the flag byte of the taking-part records set from the
 *     bitmap and loc / ent of the kept records written in stream order.
 * Loops whose trip count differs per lane have no break / continue: they are left by their condition.  Every kernel with a wave
 * primitive is run to its end by every lane.
 */
#ifndef SSG_K_MARKDUP_H
#define SSG_K_MARKDUP_H
#include "ssg_dev.h"
#include "../../include/ssgpu.h"

#define MD_OFF_MASK (((uint64_t)1 << 40) - 1)
#define MD_TAKING 1u
#define MD_PAIRED 2u
#define MD_REV 4u
#define MD_C0 0xc0u            /* flag & 0xc0, in place */
#define MD_SCORE_MAX 0x3fffffffu
#define MD_SCORE_PAIRED 0x7fffffffu   /* a paired record among the fragments of its end key */
#define MD_NEVER 4u            /* md_key_t.fl: the element is never marked */
/* mate[] of an ordinal: the other ordinal of its pair, or one of */
#define MD_NONE 0xffffffffu    /* not a paired record, or not decided */
#define MD_HELD 0xfffffffeu
#define MD_UNMATCHED 0xfffffffdu
#define MD_ORD_MAX 0xfffffff0u   /* the entries are indexed by 32 bits */

/* bits: MD_TAKING | MD_PAIRED | MD_REV | flag & 0xc0 | name bytes << 8 | library << 16 */
struct md_ent_t { uint64_t hash; int64_t u5; uint64_t name_off; int32_t tid; uint32_t score, bits, bs; };
struct md_key_t { int64_t u5a, u5b; int32_t tida, tidb; uint32_t libs, fl, score, pad; uint64_t ord_a, ord_b; };   /* libs: a | b << 16; fl: rev a | rev b << 1 | MD_NEVER */
struct md_w128_t {
	uint64_t hi, lo;   /* group << 32 | score; ~ordinal */
#ifndef SSG_EMU
	__host__ __device__
#endif
	bool operator>(const md_w128_t &o) const { return hi > o.hi || (hi == o.hi && lo > o.lo); }
};

SSG_DEVFN uint32_t md_ld32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
SSG_DEVFN bool md_same_bytes(const uint8_t *a, const uint8_t *b, uint32_t n)
{
	bool eq = true;
	for (uint32_t t = 0; t < n; ++t) eq = eq && a[t] == b[t];
	return eq;
}
SSG_DEVFN uint64_t md_name_hash(const uint8_t *name, uint32_t nl)
{
	uint64_t h = 0xcbf29ce484222325ull;   /* FNV-1a over the name, then a finishing mix: the low bits are what a narrow hash_bits keeps */
	for (uint32_t t = 0; t < nl; ++t) { h ^= name[t]; h *= 0x100000001b3ull; }
	h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
	return h;
}
/* the lanes of the wave for which p holds, added to *ctr by one lane (every lane of the wave calls it) */
SSG_DEVFN void md_count(unsigned long long *ctr, bool p, uint32_t each)
{
	const unsigned long long b = wv_ballot(p);
	if (wv_lane() == 0 && b) atomicAdd(ctr, (unsigned long long)__popcll(b) * each);
}

__global__ void __launch_bounds__(256) ssg_k_md_ends(const uint8_t *chunk, const uint64_t *loc, uint32_t n, const uint8_t *rg_ids, const uint32_t *rg_off, const uint16_t *lib_of_rg, int32_t n_rg,
                                                     md_ent_t *ent, uint32_t *nlen, unsigned long long *bad)
{
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p >= n) return;
	const uint64_t off = loc[p] & MD_OFF_MASK;
	const uint8_t *rec = chunk + off, *body = rec + 4;
	uint32_t x[6]; memcpy(x, rec, 24);   /* block_size, tid, pos, bin_mq_nl, flag_nc, l_seq: the scan has seen that 4 + block_size >= 36 bytes lie inside */
	const uint32_t bs = x[0], lq = x[3] & 0xffu, nc = x[4] & 0xffffu, flag = x[4] >> 16, l = x[5];
	uint64_t a = 32u + (uint64_t)lq + 4u * (uint64_t)nc + ((uint64_t)l + 1u) / 2u + (uint64_t)l;
	const uint64_t e = bs;
	const bool good = a <= e;
	if (!good) atomicMin(bad, (unsigned long long)off);
	const bool taking = good && !(flag & 0x904u) && nc > 0, rev = (flag & 0x10u) != 0;
	const uint32_t nl = lq ? lq - 1u : 0u;
	/* the CIGAR: the clips before the first other operation, the clips behind the last one, the reference span */
	int64_t lead = 0, trail = 0, span = 0; bool in_lead = true;
	const uint8_t *cig = body + 32 + lq;
	for (uint32_t k = 0; k < (taking ? nc : 0u); ++k) {
		const uint32_t c = md_ld32(cig + 4 * (uint64_t)k), op = c & 0xfu; const int64_t len = (int64_t)(c >> 4);
		const bool clip = op == 4u || op == 5u;
		in_lead = in_lead && clip;
		if (in_lead) lead += len;
		trail = clip ? trail + len : 0;
		if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) span += len;
	}
	const int64_t pos = (int64_t)(int32_t)x[2];
	const int64_t u5 = rev ? pos + span - 1 + trail : pos - lead;
	/* the aux area, as ssg_k_b2f_facts walks it: an unknown type (`d' among them), a Z / H without its NUL and a B without its five bytes end the walk */
	uint32_t rgo = 0, rgl = 0;
	bool go = taking && n_rg > 0 && a + 3 <= e;
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
			if (!stop && t0 == 'R' && t1 == 'G' && ty == 'Z') { rgo = (uint32_t)a; rgl = (uint32_t)(q - a); }
			sz = q - a + 1;
		} else if (ty == 'B') {
			stop = a + 5 > e;
			if (!stop) {
				const uint8_t st = body[a]; const uint64_t cnt = md_ld32(body + a + 1);
				sz = 5 + ((st == 'c' || st == 'C') ? 1u : (st == 's' || st == 'S') ? 2u : 4u) * cnt;
			}
		} else stop = true;
		a += sz;
		go = !stop && a + 3 <= e;
	}
	uint32_t lib = 0; bool found = false;
	for (int32_t g = 0; g < (rgl ? n_rg : 0); ++g) {
		const uint32_t o = rg_off[g], gl = rg_off[g + 1] - o;
		if (!found && gl == rgl && md_same_bytes(rg_ids + o, body + rgo, gl)) { lib = lib_of_rg[g]; found = true; }
	}
	const bool paired = taking && (flag & 1u) && !(flag & 8u);
	md_ent_t t;
	t.hash = md_name_hash(body + 32, good ? nl : 0u); t.u5 = taking ? u5 : 0; t.name_off = 0; t.tid = (int32_t)x[1]; t.score = 0; t.bs = bs;
	t.bits = (taking ? MD_TAKING : 0u) | (paired ? MD_PAIRED : 0u) | (rev ? MD_REV : 0u) | (flag & MD_C0) | nl << 8 | lib << 16;
	ent[p] = t;
	nlen[p] = paired ? nl : 0u;
}

/* noff[i]: where record i's name begins in `names' (the exclusive sum of nlen); base: where `names' will lie in the arena */
__global__ void __launch_bounds__(256) ssg_k_md_score(const uint8_t *chunk, const uint64_t *loc, uint32_t n, const uint64_t *noff, uint64_t base, md_ent_t *ent, uint8_t *names, uint64_t names_len)
{
	const uint32_t p = blockIdx.x * 16u + (threadIdx.x >> 4), sl = threadIdx.x & 15u;
	const bool act = p < n;
	uint64_t sum = 0;
	uint32_t bits = 0;
	if (act) bits = ent[p].bits;
	if (act && (bits & MD_TAKING)) {
		const uint64_t off = loc[p] & MD_OFF_MASK;
		const uint8_t *rec = chunk + off;
		const uint32_t lq = rec[12], nc = md_ld32(rec + 16) & 0xffffu, l = md_ld32(rec + 20);
		const uint64_t q0 = off + 36u + lq + 4u * (uint64_t)nc + ((uint64_t)l + 1u) / 2u, q1 = q0 + l;   /* the qualities: chunk bytes q0 .. q1 */
		for (uint64_t w = (q0 >> 2) + sl; 4 * w < q1; w += 16) {
			const uint32_t v = md_ld32(chunk + 4 * w);
			SSG_UNROLL
			for (uint32_t t = 0; t < 4; ++t) {
				const uint64_t at = 4 * w + t; const uint32_t q = v >> (8 * t) & 0xffu;
				if (at >= q0 && at < q1 && q >= 15u) sum += q;
			}
		}
		if (bits & MD_PAIRED) {
			const uint32_t nl = bits >> 8 & 0xffu; const uint64_t o = noff[p];
			for (uint32_t t = sl; t < nl; t += 16) if (o + t < names_len) names[o + t] = rec[36 + t];
		}
	}
	SSG_UNROLL
	for (int d = 1; d < 16; d <<= 1) sum += (uint64_t)wv_shfl64_xor((long long)sum, d);
	if (act && sl == 0) {
		ent[p].score = sum > MD_SCORE_MAX ? MD_SCORE_MAX : (uint32_t)sum;
		if (bits & MD_PAIRED) ent[p].name_off = base + noff[p];
	}
}

/* out[0] |= u5, out[1] |= tid, out[2] |= library of every taking-part entry */
__global__ void __launch_bounds__(256) ssg_k_md_bits(const md_ent_t *ent, uint64_t n, unsigned long long *out)
{
	uint64_t u = 0, t = 0, b = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
		const md_ent_t e = ent[i];
		if (e.bits & MD_TAKING) { u |= (uint64_t)e.u5; t |= (uint32_t)e.tid; b |= e.bits >> 16; }
	}
	SSG_UNROLL
	for (int d = 1; d < 64; d <<= 1) { u |= (uint64_t)wv_shfl64_xor((long long)u, d); t |= (uint64_t)wv_shfl64_xor((long long)t, d); b |= (uint64_t)wv_shfl64_xor((long long)b, d); }
	if (wv_lane() == 0) { if (u) atomicOr(out, (unsigned long long)u); if (t) atomicOr(out + 1, (unsigned long long)t); if (b) atomicOr(out + 2, (unsigned long long)b); }
}

/* which entries the two selections take: sel_p the paired ones, sel_t the taking-part ones; idx[i] = i */
__global__ void __launch_bounds__(256) ssg_k_md_classes(const md_ent_t *ent, uint32_t n, uint8_t *sel_p, uint8_t *sel_t, uint32_t *idx, uint32_t *mate, unsigned long long *counts)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	const bool act = i < n;
	uint32_t bits = 0;
	if (act) { bits = ent[i].bits; sel_p[i] = bits & MD_PAIRED ? 1 : 0; sel_t[i] = bits & MD_TAKING ? 1 : 0; idx[i] = i; mate[i] = MD_NONE; }
	md_count(counts + SSG_MD_TAKING_PART, act && (bits & MD_TAKING), 1);
	md_count(counts + SSG_MD_PAIRED, act && (bits & MD_PAIRED), 1);
	md_count(counts + SSG_MD_FRAGMENTS, act && (bits & MD_TAKING) && !(bits & MD_PAIRED), 1);
}

__global__ void __launch_bounds__(256) ssg_k_md_pkeys(const md_ent_t *ent, const uint32_t *ppos, uint32_t m, uint32_t n, int32_t hash_bits, uint64_t *key)
{
	const uint32_t j = blockIdx.x * 256u + threadIdx.x;
	if (j >= m) return;
	const uint32_t p = ppos[j];
	const uint64_t h = p < n ? ent[p].hash : 0;
	key[j] = hash_bits >= 64 ? h : hash_bits <= 0 ? 0 : h & (((uint64_t)1 << hash_bits) - 1);
}

__global__ void __launch_bounds__(256) ssg_k_md_join(const md_ent_t *ent, const uint8_t *names, uint64_t names_len, const uint64_t *key, const uint32_t *pos, uint32_t m, uint32_t n,
                                                     uint32_t *mate, uint32_t *flags)
{
	const uint32_t j = blockIdx.x * 256u + threadIdx.x;
	if (j >= m) return;
	const uint64_t k0 = key[j];
	if (pos[j] >= n) { atomicOr(flags, 2u); return; }
	if (j > 0 && key[j - 1] == k0) return;   /* not the start of a run */
	uint32_t len = 1; bool sane = true;
	while (len <= SSG_MARKDUP_RUN_MAX && j + len < m && key[j + len] == k0) { sane = sane && pos[j + len] < n; ++len; }
	if (len > SSG_MARKDUP_RUN_MAX) { atomicOr(flags, 1u); return; }
	for (uint32_t i = 0; i < len; ++i) sane = sane && ent[pos[j + i]].name_off + (ent[pos[j + i]].bits >> 8 & 0xffu) <= names_len;
	if (!sane) { atomicOr(flags, 2u); return; }
	for (uint32_t i = 0; i < len; ++i) {
		const uint32_t p = pos[j + i];
		const md_ent_t ep = ent[p];
		const uint32_t nl = ep.bits >> 8 & 0xffu;
		uint32_t held = MD_NONE;   /* the held record of this name: at most one */
		for (uint32_t k = 0; k < i; ++k) {
			const uint32_t q = pos[j + k];
			if (held == MD_NONE && mate[q] == MD_HELD && ent[q].hash == ep.hash && (ent[q].bits >> 8 & 0xffu) == nl && md_same_bytes(names + ent[q].name_off, names + ep.name_off, nl)) held = q;
		}
		if (held == MD_NONE) mate[p] = MD_HELD;
		else if ((ent[held].bits & MD_C0) == (ep.bits & MD_C0)) mate[p] = MD_UNMATCHED;
		else { mate[p] = held; mate[held] = p; }
	}
}

/* owner[j] = 1 where the sorted paired entry j is the later record of a pair (a kernel of its own: the run's walk has to be over in every workgroup) */
__global__ void __launch_bounds__(256) ssg_k_md_owners(const uint32_t *pos, uint32_t m, uint32_t n, const uint32_t *mate, uint8_t *owner)
{
	const uint32_t j = blockIdx.x * 256u + threadIdx.x;
	if (j >= m) return;
	const uint32_t p = pos[j];
	owner[j] = p < n && mate[p] < p ? 1 : 0;
}

SSG_DEVFN bool md_end_before(const md_ent_t &a, const md_ent_t &b)
{
	if (a.tid != b.tid) return a.tid < b.tid;
	if (a.u5 != b.u5) return a.u5 < b.u5;
	if ((a.bits & MD_REV) != (b.bits & MD_REV)) return !(a.bits & MD_REV);
	return (a.bits >> 16) < (b.bits >> 16);
}

/* own[k]: the later record of pair k */
__global__ void __launch_bounds__(256) ssg_k_md_pairs(const md_ent_t *ent, const uint32_t *mate, const uint32_t *own, uint32_t n_pairs, uint32_t n, md_key_t *key, uint32_t *idx)
{
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	if (k >= n_pairs) return;
	const uint32_t p = own[k] < n ? own[k] : 0, q = mate[p] < n ? mate[p] : 0;
	const md_ent_t ep = ent[p], eq = ent[q];
	const bool pf = md_end_before(ep, eq);
	const md_ent_t &a = pf ? ep : eq, &b = pf ? eq : ep;
	md_key_t t;
	t.u5a = a.u5; t.u5b = b.u5; t.tida = a.tid; t.tidb = b.tid; t.libs = a.bits >> 16 | (b.bits >> 16) << 16; t.fl = (a.bits & MD_REV ? 1u : 0u) | (b.bits & MD_REV ? 2u : 0u);
	t.score = ep.score + eq.score; t.pad = 0; t.ord_a = q < p ? q : p; t.ord_b = q < p ? p : q;
	key[k] = t; idx[k] = k;
}

__global__ void __launch_bounds__(256) ssg_k_md_frags(const md_ent_t *ent, const uint32_t *tpos, uint32_t m, uint32_t n, md_key_t *key, uint32_t *idx)
{
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	if (k >= m) return;
	const uint32_t p = tpos[k] < n ? tpos[k] : 0;
	const md_ent_t e = ent[p];
	md_key_t t;
	t.u5a = e.u5; t.u5b = 0; t.tida = e.tid; t.tidb = 0; t.libs = e.bits >> 16; t.fl = (e.bits & MD_REV ? 1u : 0u) | (e.bits & MD_PAIRED ? MD_NEVER : 0u);
	t.score = e.bits & MD_PAIRED ? MD_SCORE_PAIRED : e.score; t.pad = 0; t.ord_a = p; t.ord_b = p;
	key[k] = t; idx[k] = k;
}

/* word 0: u5a; 1: u5b; 2: tida | tidb << 32; 3: the strands | libs << 2 */
SSG_DEVFN uint64_t md_key_word(const md_key_t &t, int32_t w)
{
	return w == 0 ? (uint64_t)t.u5a : w == 1 ? (uint64_t)t.u5b : w == 2 ? (uint64_t)(uint32_t)t.tida | (uint64_t)(uint32_t)t.tidb << 32 : (uint64_t)(t.fl & 3u) | (uint64_t)t.libs << 2;
}
__global__ void __launch_bounds__(256) ssg_k_md_word(const md_key_t *key, const uint32_t *idx, uint32_t m, int32_t w, uint64_t *out)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= m) return;
	const uint32_t k = idx[i] < m ? idx[i] : 0;
	out[i] = md_key_word(key[k], w);
}

__global__ void __launch_bounds__(256) ssg_k_md_heads(const md_key_t *key, const uint32_t *idx, uint32_t m, uint32_t *head)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= m) return;
	bool h = i == 0;
	if (i > 0) {
		const md_key_t a = key[idx[i] < m ? idx[i] : 0], b = key[idx[i - 1] < m ? idx[i - 1] : 0];
		h = a.u5a != b.u5a || a.u5b != b.u5b || a.tida != b.tida || a.tidb != b.tidb || a.libs != b.libs || (a.fl & 3u) != (b.fl & 3u);
	}
	head[i] = h ? 1u : 0u;
}

/* before[i]: the heads before element i */
SSG_DEVFN md_w128_t md_pack(const md_key_t &t, uint32_t g) { md_w128_t w; w.hi = (uint64_t)g << 32 | t.score; w.lo = ~t.ord_a; return w; }
__global__ void __launch_bounds__(256) ssg_k_md_pack(const md_key_t *key, const uint32_t *idx, const uint32_t *head, const uint32_t *before, uint32_t m, md_w128_t *w)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= m) return;
	w[i] = md_pack(key[idx[i] < m ? idx[i] : 0], before[i] + head[i] - 1u);
}
__global__ void __launch_bounds__(256) ssg_k_md_best(const md_w128_t *run, const uint32_t *head, const uint32_t *before, uint32_t m, md_w128_t *best)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= m) return;
	const uint32_t g = before[i] + head[i] - 1u;
	if ((i + 1 == m || head[i + 1]) && g < m) best[g] = run[i];
}
/* c_pairs / c_frags: which of the two counters an element adds to (the other pointer is NULL) */
__global__ void __launch_bounds__(256) ssg_k_md_mark(const md_key_t *key, const uint32_t *idx, const uint32_t *head, const uint32_t *before, const md_w128_t *best, uint32_t m, uint64_t n,
                                                     uint32_t *bitmap, unsigned long long *c_pairs, unsigned long long *c_frags)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	bool dup = false;
	if (i < m) {
		const md_key_t t = key[idx[i] < m ? idx[i] : 0];
		const uint32_t g = before[i] + head[i] - 1u;
		const md_w128_t w = md_pack(t, g), b = best[g < m ? g : 0];
		dup = !(t.fl & MD_NEVER) && (w.hi != b.hi || w.lo != b.lo);
		if (dup && t.ord_a < n) atomicOr(bitmap + (t.ord_a >> 5), 1u << (t.ord_a & 31u));
		if (dup && t.ord_b < n) atomicOr(bitmap + (t.ord_b >> 5), 1u << (t.ord_b & 31u));
	}
	if (c_pairs) md_count(c_pairs, dup, 2);
	if (c_frags) md_count(c_frags, dup, 1);
}

/* the second pass: ordinal ord0 + i for record i of the chunk */
__global__ void __launch_bounds__(256) ssg_k_md_apply(uint8_t *chunk, const uint64_t *loc, const ssg_bam_ent_t *ent, int64_t n_rec, const md_ent_t *first, const uint32_t *bitmap, uint64_t ord0, int32_t remove,
                                                      uint32_t *cnt, unsigned long long *bad, const uint64_t *base, uint64_t n_out, uint64_t *out_loc, ssg_bam_ent_t *out_ent)
{
	__shared__ uint32_t s_kept[4];   /* the kept lanes of the workgroup's four waves */
	const int64_t i = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
	const bool act = i < n_rec;
	uint64_t l = 0; ssg_bam_ent_t e;
	e.tid = e.pos = e.end = 0; e.flag = e.len = e.pad = 0;
	bool keep = false, taking = false, dup = false;
	uint8_t *rec = chunk;
	if (act) {
		l = loc[i]; e = ent[i];
		rec = chunk + (l & MD_OFF_MASK);
		const uint64_t ord = ord0 + (uint64_t)i;
		const md_ent_t f = first[ord];
		taking = (f.bits & MD_TAKING) != 0;
		dup = taking && (bitmap[ord >> 5] >> (ord & 31u) & 1u);
		keep = !(remove && dup);
		if (!base) {   /* the scan has seen that l_qname bytes lie inside the record */
			const uint32_t bs = md_ld32(rec), lq = rec[12];
			if (bs != f.bs || md_name_hash(rec + 36, lq ? lq - 1u : 0u) != f.hash) atomicMin(bad, (unsigned long long)ord);
		}
	}
	const unsigned long long kept = wv_ballot(keep);
	const int wave = (int)(threadIdx.x >> 6);
	if (wv_lane() == 0) s_kept[wave] = (uint32_t)__popcll(kept);
	__syncthreads();
	if (!base) {
		if (threadIdx.x == 0) cnt[blockIdx.x] = s_kept[0] + s_kept[1] + s_kept[2] + s_kept[3];
	} else if (act) {
		if (taking) {   /* 0x400: bit 2 of the flag's high byte, byte 19 of the record */
			const uint8_t b = rec[19], nb = (uint8_t)((b & ~4u) | (dup ? 4u : 0u));
			if (nb != b) rec[19] = nb;
			e.flag = (e.flag & ~0x400u) | (dup ? 0x400u : 0u);
		}
		if (keep) {
			uint64_t w = base[blockIdx.x] + (uint64_t)wv_rank_of(kept);
			if (wave > 0) w += s_kept[0];
			if (wave > 1) w += s_kept[1];
			if (wave > 2) w += s_kept[2];
			if (w < n_out) { out_loc[w] = l; out_ent[w] = e; }
		}
	}
}
#endif
