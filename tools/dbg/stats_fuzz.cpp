/*
 * stats_fuzz.cpp -- memory safety and exactness of ssg_stats_* (k_stats.h) on the host emulation and under the sanitizers (never on a GPU: a stand-alone program,
 * `make fuzz-stats` builds and runs it).  3000 seeded cases: a stream of BAM-shaped records -- every flag bit, CIGARs of every operation code (unknown ones and
 * lengths of 0 among them) that do or do not add up to l_seq, an l_seq of 0, sequences of every 4-bit code, qualities of every byte, names with and without NUL,
 * aux areas of every type that end where they should, are cut short or are noise, insert sizes up to INT32_MIN -- in one to three chunks, each exactly as long
 * as its records plus the store's 16 bytes of slack (a heap block of the emulation: the sanitizer sees a load behind it); sorted or not; with small max_len,
 * n_isize and coverage bins, spans from 1 position on, and LDS tiles and slabs of every size.  In every fifth case one record is broken: an l_seq that leaves the
 * record, a mapped record without CIGAR, hard clips beyond max_len, or an insertion outside the cycles.  A plain C++ loop over the records says what must come
 * back -- every scalar and table, or the refusal's code with the object as it was before the push; every refusal of the arguments and of the state is asked for
 * once a case.  The sanitizers watch the rest.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include <algorithm>
#include <map>
#include <string>
#include <vector>
#include "../../include/ssgpu.h"

thread_local std::string ssg_err_msg;      /* what ssgpu_core.cpp defines for the library */
thread_local int ssg_cur_dev = 0;
thread_local int ssg_lane = 0;

typedef std::vector<uint8_t> bytes_t;
static uint64_t rng_s = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rng_s ^= rng_s << 13; rng_s ^= rng_s >> 7; rng_s ^= rng_s << 17; return (uint32_t)(rng_s >> 16); }
static long n_fail = 0;
#define EXPECT(c, ...) do { if (!(c)) { if (++n_fail < 20) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static void put32(bytes_t &b, uint32_t v) { b.insert(b.end(), (const uint8_t*)&v, (const uint8_t*)&v + 4); }
static void aux_area(bytes_t &b)
{
	const uint32_t kind = rnd() % 8;
	if (kind == 0) return;
	if (kind == 1) { for (uint32_t i = rnd() % 12; i > 0; --i) b.push_back((uint8_t)rnd()); return; }   /* noise */
	for (uint32_t n = 1 + rnd() % 5; n > 0; --n) {
		const bool nm = rnd() % 3 == 0;
		b.push_back(nm ? 'N' : 'X'); b.push_back(nm ? 'M' : (uint8_t)('a' + rnd() % 26));
		static const char types[] = "AcCsSiIfZHBd";
		const char ty = nm && rnd() % 4 ? "cCsSiI"[rnd() % 6] : types[rnd() % 12];
		b.push_back((uint8_t)ty);
		uint32_t sz = ty == 'A' || ty == 'c' || ty == 'C' ? 1 : ty == 's' || ty == 'S' ? 2 : ty == 'd' ? 8 : 4;
		if (ty == 'Z' || ty == 'H') { for (uint32_t i = rnd() % 6; i > 0; --i) b.push_back((uint8_t)('0' + rnd() % 10)); if (rnd() % 10) b.push_back(0); continue; }
		if (ty == 'B') { const char st = "cCsSiIf"[rnd() % 7]; const uint32_t cnt = rnd() % 4; b.push_back((uint8_t)st); put32(b, rnd() % 30 == 0 ? 0xffffffffu : cnt); sz = cnt * (st == 'c' || st == 'C' ? 1 : st == 's' || st == 'S' ? 2 : 4); }
		if (rnd() % 12 == 0 && sz) sz = rnd() % sz;   /* cut short */
		for (uint32_t i = 0; i < sz; ++i) b.push_back(rnd() % 3 ? (uint8_t)(rnd() % 4) : (uint8_t)rnd());
	}
}
static bool g_tidy = false;   /* two cases of three: CIGARs that add up to l_seq and stay inside max_len, so that a chunk of a hundred records is not refused by accident */
static void record(bytes_t &s, int32_t tid, int32_t pos, uint32_t max_len)
{
	const uint32_t l_qname = rnd() % 20 == 0 ? 255 : rnd() % 20 == 0 ? 0 : 1 + rnd() % 6, nc = rnd() % 10 == 0 ? 0 : 1 + rnd() % (rnd() % 8 == 0 ? (g_tidy ? 8 : 40) : 5);
	uint32_t flag = 0;
	static const uint32_t bits[12] = { 1, 2, 4, 8, 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x400, 0x800 }; static const uint32_t odds[12] = { 2, 2, 8, 10, 2, 2, 2, 3, 12, 8, 8, 12 };
	for (int k = 0; k < 12; ++k) if (rnd() % odds[k] == 0) flag |= bits[k];
	if (nc == 0 && (g_tidy || rnd() % 16)) flag |= 4;   /* (a mapped record without CIGAR is a refusal) */
	bytes_t body; uint32_t qlen = 0;
	for (uint32_t i = 0; i < l_qname; ++i) body.push_back(i + 1 == l_qname && rnd() % 8 ? 0 : rnd() % 30 == 0 ? 0 : (uint8_t)('a' + rnd() % 26));
	for (uint32_t i = 0; i < nc; ++i) {
		const uint32_t op = rnd() % 16 == 0 ? 9 + rnd() % 7 : rnd() % 2 == 0 ? rnd() % 9 : 0, len = rnd() % 12 == 0 ? 0 : op == 5 ? rnd() % 3 : g_tidy ? 1 + rnd() % (max_len / 16 + 1) : rnd() % 40 == 0 ? 290 + rnd() % 20 : 1 + rnd() % (max_len / 8 + 1);
		put32(body, len << 4 | op);
		if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8 || (g_tidy && op > 8)) qlen += len;
	}
	uint32_t l_seq = rnd() % 8 == 0 ? 0 : !g_tidy && rnd() % 40 == 0 ? rnd() % (qlen + 2) : qlen;
	if (l_seq > max_len) l_seq = rnd() % 40 == 0 ? max_len + 1 : 1 + rnd() % max_len;
	const uint32_t sk = rnd() % 3;
	for (uint32_t i = 0; i < (l_seq + 1) / 2; ++i) body.push_back(sk == 0 ? (uint8_t)rnd() : (uint8_t)((1u << rnd() % 4) << 4 | 1u << rnd() % 4));
	const uint32_t qk = rnd() % 4;
	for (uint32_t i = 0; i < l_seq; ++i) body.push_back(qk == 0 ? 0xff : qk == 1 ? (uint8_t)rnd() : (uint8_t)(rnd() % 42));
	aux_area(body);
	static const int32_t sizes[8] = { 0, 1, -1, 300, -300, INT32_MIN, INT32_MAX, 7999 };
	const uint32_t core[9] = { 32 + (uint32_t)body.size(), (uint32_t)tid, (uint32_t)pos, l_qname | (rnd() % 3 ? 30u : 0u) << 8, flag << 16 | nc, l_seq,
	                           rnd() % 4 ? (uint32_t)tid : rnd() % 3, (uint32_t)(pos + (int32_t)(rnd() % 600) - 300), (uint32_t)(rnd() % 3 ? sizes[rnd() % 8] : (int32_t)(rnd() % 900) - 450) };
	s.insert(s.end(), (const uint8_t*)core, (const uint8_t*)core + 36);
	s.insert(s.end(), body.begin(), body.end());
}

/* ---- the contract in plain C++ ---- */
struct filter_t { const char *what; std::vector<ssg_bam_fop_t> prog; bool (*keeps)(uint32_t flag, uint32_t mapq); };
static ssg_bam_fop_t fop(int op, int arg, int32_t v) { ssg_bam_fop_t f; f.op = (uint8_t)op; f.arg = (uint8_t)arg; f.pad = 0; f.value = v; return f; }
static std::vector<filter_t> filters()
{
	std::vector<filter_t> F;
	F.push_back({ "everything", {}, [](uint32_t, uint32_t) { return true; } });
	F.push_back({ "not duplicate", { fop(SSG_FOP_FLAG, 0, 0x400), fop(SSG_FOP_NOT, 0, 0) }, [](uint32_t f, uint32_t) { return !(f & 0x400); } });
	F.push_back({ "paired and mapq", { fop(SSG_FOP_FLAG, 0, 1), fop(SSG_FOP_GE, SSG_FLD_MAPQ, 1), fop(SSG_FOP_AND, 0, 0) }, [](uint32_t f, uint32_t q) { return (f & 1) && q >= 1; } });
	F.push_back({ "nothing", { fop(SSG_FOP_LT, SSG_FLD_SEQ_LEN, 0) }, [](uint32_t, uint32_t) { return false; } });
	return F;
}
struct plain_t {
	ssg_stats_opt_t o; int64_t n_cov; size_t rows;
	std::vector<uint64_t> sc, quals, bases, gc, isz, rl, id, ic, cov;
	std::map<uint64_t, int64_t> ends; bool have_last; uint64_t last;
	void init(const ssg_stats_opt_t &o_, int64_t n_cov_)
	{
		o = o_; n_cov = n_cov_; rows = (size_t)o.max_len + 1;
		sc.assign(SSG_ST_N, 0); quals.assign(2 * rows * 256, 0); bases.assign(rows * 6, 0); gc.assign(2 * SSG_STATS_NGC, 0); isz.assign(3 * (size_t)o.n_isize, 0); rl.assign(rows, 0);
		id.assign(2 * SSG_STATS_NINDEL, 0); ic.assign(4 * rows, 0); cov.assign((size_t)n_cov, 0); sc[SSG_ST_SORTED] = 1; have_last = false; last = 0;
	}
};
static int64_t first_nm(const uint8_t *b, uint64_t a, uint64_t e)
{
	while (a + 3 <= e) {
		const uint8_t t0 = b[a], t1 = b[a + 1], ty = b[a + 2]; a += 3;
		uint64_t sz;
		if (ty == 'A' || ty == 'c' || ty == 'C') sz = 1; else if (ty == 's' || ty == 'S') sz = 2; else if (ty == 'i' || ty == 'I' || ty == 'f') sz = 4;
		else if (ty == 'Z' || ty == 'H') { uint64_t q = a; while (q < e && b[q]) ++q; if (q >= e) return 0; sz = q - a + 1; }
		else if (ty == 'B') { if (a + 5 > e) return 0; uint32_t cnt; memcpy(&cnt, b + a + 1, 4); const uint8_t st = b[a]; sz = 5 + (uint64_t)(st == 'c' || st == 'C' ? 1 : st == 's' || st == 'S' ? 2 : 4) * cnt; }
		else return 0;
		if (a + sz > e) return 0;
		if (t0 == 'N' && t1 == 'M') {
			if (ty == 'c') return (int8_t)b[a];
			if (ty == 'C') return b[a];
			if (ty == 's') { int16_t v; memcpy(&v, b + a, 2); return v; }
			if (ty == 'S') { uint16_t v; memcpy(&v, b + a, 2); return v; }
			if (ty == 'i' || ty == 'I') { int32_t v; memcpy(&v, b + a, 4); return v; }
			return 0;
		}
		a += sz;
	}
	return 0;
}
/* one chunk into a copy of P; the code a push of it must return (the first refusal in the library's order of precedence), P untouched when it is not 0 */
static int plain_push(const bytes_t &s, const filter_t &F, plain_t &P, uint64_t &n_rec, uint64_t &desc)
{
	plain_t Q = P; n_rec = desc = 0;
	bool e_fit = false, e_long = false, e_nocig = false, e_cyc = false;
	std::vector<uint64_t> keys; std::vector<uint32_t> lens;
	const int64_t L = P.o.max_len;
	for (uint64_t o = 0; o < s.size(); ) {
		uint32_t x[9]; memcpy(x, s.data() + o, 36);
		const uint64_t bs = x[0], lq = x[3] & 0xff, nc = x[4] & 0xffff, l = x[5];
		const uint32_t flag = x[4] >> 16, mapq = x[3] >> 8 & 0xff;
		const uint8_t *body = s.data() + o + 4, *name = body + 32, *cig = name + lq, *seq = cig + 4 * nc, *qual = seq + (l + 1) / 2;
		const uint64_t aux0 = 32 + lq + 4 * nc + (l + 1) / 2 + l;
		o += 4 + bs; ++n_rec;
		if (aux0 > bs) { e_fit = true; continue; }
		if (!F.keeps(flag, mapq)) { ++Q.sc[SSG_ST_FILTERED]; continue; }
		uint64_t nl = 0; while (nl < lq && name[nl]) ++nl;
		Q.sc[SSG_ST_CHK_NAMES] = (uint32_t)(Q.sc[SSG_ST_CHK_NAMES] + crc32(0, name, (uInt)nl));
		if (l) { Q.sc[SSG_ST_CHK_READS] = (uint32_t)(Q.sc[SSG_ST_CHK_READS] + crc32(0, seq, (uInt)((l + 1) / 2))); Q.sc[SSG_ST_CHK_QUALS] = (uint32_t)(Q.sc[SSG_ST_CHK_QUALS] + crc32(0, qual, (uInt)((l + 1) / 2))); }
		if (flag & 0x100) { ++Q.sc[SSG_ST_SECONDARY]; continue; }
		if (!l) continue;
		if (flag & 0x400) { ++Q.sc[SSG_ST_DUP]; Q.sc[SSG_ST_DUP_LEN] += l; }
		int64_t hard = 0;
		for (uint64_t k = 0; k < nc; ++k) { uint32_t v; memcpy(&v, cig + 4 * k, 4); if ((v & 15) == 5) hard += v >> 4; }
		const int64_t un = (int64_t)l + hard;
		const bool rev = flag & 0x10, mapped = !(flag & 4), both = (flag & 1) && !(flag & 4) && !(flag & 8);
		if (mapped && nc == 0) e_nocig = true;
		if (mapped) {   /* count_indels: the cycles are judged whatever the length */
			const int f1 = flag & 0x40 ? 0 : 1; int64_t cyc = 0;
			for (uint64_t k = 0; k < nc; ++k) {
				uint32_t v; memcpy(&v, cig + 4 * k, 4); const uint32_t op = v & 15; const int64_t n = v >> 4;
				if (!n) continue;
				if (op == 1) { const int64_t ix = rev ? (int64_t)l - cyc - n : cyc; if (ix < 0 || ix > L) e_cyc = true; else if (un <= L) { ++Q.ic[(size_t)f1 * Q.rows + (size_t)ix]; if (n <= SSG_STATS_NINDEL) ++Q.id[(size_t)n - 1]; } cyc += n; }
				else if (op == 2) { const int64_t ix = rev ? (int64_t)l - cyc - 1 : cyc - 1; if (ix > L) e_cyc = true; else if (ix >= 0 && un <= L) { ++Q.ic[(size_t)(2 + f1) * Q.rows + (size_t)ix]; if (n <= SSG_STATS_NINDEL) ++Q.id[SSG_STATS_NINDEL + (size_t)n - 1]; } }
				else if (op != 3 && op != 5 && op != 6) cyc += n;
			}
		}
		if (un > L) { e_long = true; continue; }
		Q.sc[SSG_ST_MAX_LEN] = std::max<uint64_t>(Q.sc[SSG_ST_MAX_LEN], (uint64_t)un);
		if (!(flag & 0x900)) {
			const int fr = flag & 0x80 ? 1 : 0;
			++Q.rl[(size_t)un]; Q.sc[SSG_ST_TOTAL_LEN] += l; Q.sc[SSG_ST_QCFAIL] += flag & 0x200 ? 1 : 0; Q.sc[SSG_ST_PAIRED] += flag & 1; ++Q.sc[fr ? SSG_ST_LAST : SSG_ST_FIRST];
			uint64_t g = 0;
			for (uint64_t i = 0; i < l; ++i) {
				const uint64_t cyc = rev ? l - 1 - i : i; const uint32_t code = seq[i / 2] >> (i & 1 ? 0 : 4) & 15, q = qual[i];
				++Q.bases[cyc * 6 + (code == 1 ? 0 : code == 2 ? 1 : code == 4 ? 2 : code == 8 ? 3 : code == 15 ? 4 : 5)];
				g += code == 2 || code == 4;
				++Q.quals[((size_t)fr * Q.rows + cyc) * 256 + q]; Q.sc[SSG_ST_SUM_QUAL] += q; Q.sc[SSG_ST_MAX_QUAL] = std::max<uint64_t>(Q.sc[SSG_ST_MAX_QUAL], q);
			}
			for (uint64_t k = g * 199 / l; k < std::min<uint64_t>((g + 1) * 199 / l, 199); ++k) ++Q.gc[(size_t)fr * SSG_STATS_NGC + k];
			if (!mapped) ++Q.sc[SSG_ST_UNMAPPED];
			else {
				Q.sc[SSG_ST_BASES_MAPPED] += l; Q.sc[SSG_ST_MQ0] += mapq == 0; ++Q.sc[both ? SSG_ST_PAIRED_MAPPED : SSG_ST_SINGLE];
				if (both) { Q.sc[SSG_ST_PROPER] += flag & 2 ? 1 : 0; Q.sc[SSG_ST_ANOMALOUS] += x[1] != x[6]; }
			}
		}
		if (!mapped) continue;
		if (both) {
			int64_t a = (int32_t)x[8]; a = a < 0 ? -a : a; a = std::min<int64_t>(a, P.o.n_isize - 1);
			if (a > 0 || x[1] == x[6]) {
				const int64_t d = (int64_t)(int32_t)x[7] - (int64_t)(int32_t)x[2]; const int sf = flag & 0x40 ? 1 : -1, sw = rev ? -1 : 1, sm = flag & 0x20 ? -1 : 1;
				if (sw * sm > 0) ++Q.isz[2 * (size_t)P.o.n_isize + (size_t)a];
				else if (sf * d > 0) ++Q.isz[(sf * sw > 0 ? 0 : 1) * (size_t)P.o.n_isize + (size_t)a];
				else if (sf * d < 0) ++Q.isz[(sf * sw > 0 ? 1 : 0) * (size_t)P.o.n_isize + (size_t)a];
			}
		}
		Q.sc[SSG_ST_MISMATCHES] += (uint64_t)first_nm(body, aux0, bs);
		for (uint64_t k = 0; k < nc; ++k) { uint32_t v; memcpy(&v, cig + 4 * k, 4); if ((v & 15) < 2) Q.sc[SSG_ST_BASES_CIGAR] += v >> 4; }
		if (nc) { keys.push_back((uint64_t)x[1] << 32 | x[2]); lens.push_back((uint32_t)l); }
	}
	if (e_fit || e_nocig || e_cyc) { n_rec = 0; return e_fit ? SSG_EIO : e_long ? SSG_ERANGE : SSG_EIO; }
	if (e_long) { n_rec = 0; return SSG_ERANGE; }
	if (Q.sc[SSG_ST_SORTED]) {
		for (size_t k = 0; k < keys.size(); ++k) { if ((k > 0 || Q.have_last) && keys[k] < (k > 0 ? keys[k - 1] : Q.last)) ++desc; }
		if (desc) { Q.sc[SSG_ST_SORTED] = 0; Q.ends.clear(); }
		else for (size_t k = 0; k < keys.size(); ++k) { ++Q.ends[keys[k]]; --Q.ends[keys[k] + lens[k]]; }   /* (a read over pos 2^32 would carry into the tid: none is made) */
		if (!keys.empty()) { Q.last = keys.back(); Q.have_last = true; }
	}
	P = Q;
	return 0;
}
static void plain_finish(plain_t &P)
{
	if (!P.sc[SSG_ST_SORTED]) return;
	int64_t depth = 0; uint64_t at = 0;
	for (const auto &e : P.ends) {
		if (depth) P.cov[(size_t)(depth < P.o.cov_min ? 0 : depth > P.o.cov_max ? P.n_cov - 1 : 1 + (depth - P.o.cov_min) / P.o.cov_step)] += e.first - at;   /* coverage_idx */
		depth += e.second; at = e.first;
	}
}

int main()
{
	const std::vector<filter_t> F = filters();
	long n_push = 0, n_refused = 0, n_unsorted = 0; uint64_t n_bases = 0;
	for (int c = 0; c < 3000; ++c) {
		rng_s = 0x9e3779b97f4a7c15ull ^ ((uint64_t)(c + 1) * 0x2545f4914f6cdd1dull);
		const filter_t &flt = F[rnd() % F.size()];
		static const char *const TILES[] = { "1", "3", "31", "32", 0 }, *const SLABS[] = { "1", "7", "100", 0 };
		const char *const tile = TILES[rnd() % 5], *const slab = SLABS[rnd() % 4];
		if (tile) setenv("SSG_STATS_TILE", tile, 1); else unsetenv("SSG_STATS_TILE");
		if (slab) setenv("SSG_STATS_SLAB", slab, 1); else unsetenv("SSG_STATS_SLAB");
		ssg_stats_opt_t o; o.max_len = 48 + (int32_t)(rnd() % 400); g_tidy = c % 3 != 0; o.n_isize = rnd() % 4 == 0 ? 1 + (int32_t)(rnd() % 10) : 8000; o.cov_min = (int32_t)(rnd() % 3); o.cov_max = o.cov_min + (int32_t)(rnd() % 30);
		o.cov_step = 1 + (int32_t)(rnd() % 5); o.span = rnd() % 5 == 0 ? 0 : 1 + (int32_t)(rnd() % 700);
		ssg_stats_opt_t rounded = o;   /* as init_stat_structs rounds them */
		if (rounded.cov_step > rounded.cov_max - rounded.cov_min + 1) { rounded.cov_step = rounded.cov_max - rounded.cov_min; if (rounded.cov_step <= 0) rounded.cov_step = 1; }
		const int64_t n_cov = 3 + (rounded.cov_max - rounded.cov_min) / rounded.cov_step;
		rounded.cov_max = rounded.cov_min + ((rounded.cov_max - rounded.cov_min) / rounded.cov_step + 1) * rounded.cov_step - 1;
		EXPECT(ssg_stats_ncov(&o) == n_cov, "case %d: %lld bins, wanted %lld", c, (long long)ssg_stats_ncov(&o), (long long)n_cov);
		/* the chunks */
		const uint32_t n = rnd() % 300, spread = rnd() % 3 == 0 ? 5000 : 400, n_chunks = 1 + rnd() % 3; const bool sorted = rnd() % 4 != 0;
		std::vector<std::pair<int32_t, int32_t> > at;
		for (uint32_t i = 0; i < n; ++i) at.push_back(std::make_pair((int32_t)(rnd() % 16 == 0 ? 3 : rnd() % 3), (int32_t)(rnd() % spread)));
		if (sorted) std::sort(at.begin(), at.end());
		std::vector<bytes_t> chunk(n_chunks); std::vector<std::vector<uint64_t> > starts(n_chunks);
		for (uint32_t i = 0; i < n; ++i) { const uint32_t k = (uint32_t)((uint64_t)i * n_chunks / n); starts[k].push_back(chunk[k].size()); record(chunk[k], at[i].first, at[i].second, (uint32_t)o.max_len); }
		if (c % 5 == 0 && n > 0) {   /* one broken record */
			uint32_t k = rnd() % n_chunks; while (starts[k].empty()) k = (k + 1) % n_chunks;
			bytes_t &s = chunk[k]; const uint64_t ro = starts[k][rnd() % starts[k].size()]; uint32_t x[6]; memcpy(x, s.data() + ro, 24);
			const uint32_t how = rnd() % 4, lq = x[3] & 0xff, nc = x[4] & 0xffff;
			if (how == 0) { const uint32_t l = rnd() % 2 ? 0x7fffffffu : x[5] + 1 + rnd() % 60 + 2 * (x[0] - 32); memcpy(s.data() + ro + 20, &l, 4); }
			else if (how == 1 && nc > 0) { const uint32_t v = ((uint32_t)o.max_len + rnd() % 3) << 4 | 5u; memcpy(s.data() + ro + 36 + lq, &v, 4); }
			else if (how == 2 && nc > 0) { const uint32_t v = (1u + rnd() % 5) << 4 | 1u, f = (x[4] | 0x10u << 16) & ~(0x104u << 16); memcpy(s.data() + ro + 36 + lq + 4 * (nc - 1), &v, 4); memcpy(s.data() + ro + 16, &f, 4); }
			else { const uint32_t f = x[4] & ~(0x4u << 16); memcpy(s.data() + ro + 16, &f, 4); }
		}
		ssg_recs_t *r = 0; ssg_stats_t *st = 0;
		if (ssg_recs_create(~(uint64_t)0 >> 1, &r)) { EXPECT(0, "create: %s", ssg_err_msg.c_str()); return 1; }
		{	/* what create refuses */
			ssg_stats_t *x = 0; ssg_stats_opt_t b = o; const ssg_bam_fop_t under[1] = { fop(SSG_FOP_AND, 0, 0) }, two[2] = { fop(SSG_FOP_FLAG, 0, 1), fop(SSG_FOP_FLAG, 0, 2) };
			EXPECT(ssg_stats_create(r, under, 1, &o, &x) == SSG_EINVAL && ssg_stats_create(r, two, 2, &o, &x) == SSG_EINVAL && ssg_stats_create(0, 0, 0, &o, &x) == SSG_EINVAL && ssg_stats_create(r, 0, 0, 0, &x) == SSG_EINVAL, "a bad program, store or no options were taken");
			b.max_len = 0; EXPECT(ssg_stats_create(r, 0, 0, &b, &x) == SSG_EINVAL, "max_len 0"); b = o; b.n_isize = 0; EXPECT(ssg_stats_create(r, 0, 0, &b, &x) == SSG_EINVAL, "n_isize 0");
			b = o; b.cov_step = 0; EXPECT(ssg_stats_create(r, 0, 0, &b, &x) == SSG_EINVAL && ssg_stats_ncov(&b) == -1, "cov_step 0"); b = o; b.span = -1; EXPECT(ssg_stats_create(r, 0, 0, &b, &x) == SSG_EINVAL, "span -1");
			b = o; b.cov_max = b.cov_min - 1; EXPECT(ssg_stats_create(r, 0, 0, &b, &x) == SSG_EINVAL, "cov_max < cov_min"); b = o; b.cov_min = 0; b.cov_max = 9000; b.cov_step = 1; EXPECT(ssg_stats_create(r, 0, 0, &b, &x) == SSG_EINVAL, "9003 bins");
		}
		if (ssg_stats_create(r, flt.prog.empty() ? 0 : flt.prog.data(), (int)flt.prog.size(), &o, &st)) { EXPECT(0, "create: %s", ssg_err_msg.c_str()); return 1; }
		plain_t P; P.init(rounded, n_cov);
		auto same = [&](const char *when) {
			plain_t G; G.init(rounded, n_cov);   /* exactly as long as the tables: a store behind them is the sanitizer's */
			const int rc = ssg_stats_get(st, G.sc.data(), G.quals.data(), G.bases.data(), G.gc.data(), G.isz.data(), G.rl.data(), G.id.data(), G.ic.data(), G.cov.data());
			std::vector<uint64_t> half(P.isz); for (uint64_t &v : half) v /= 2;
			EXPECT(rc == 0 && G.sc == P.sc && G.quals == P.quals && G.bases == P.bases && G.gc == P.gc && G.isz == half && G.rl == P.rl && G.id == P.id && G.ic == P.ic,
			       "case %d (%s, tile %s, slab %s, max_len %d) %s: rc %d; differ: sc %d quals %d bases %d gc %d isize %d rl %d id %d ic %d", c, flt.what, tile ? tile : "default", slab ? slab : "default", o.max_len, when, rc,
			       G.sc != P.sc, G.quals != P.quals, G.bases != P.bases, G.gc != P.gc, G.isz != half, G.rl != P.rl, G.id != P.id, G.ic != P.ic);
			if (G.sc != P.sc && n_fail < 20) for (int k = 0; k < SSG_ST_N; ++k) if (G.sc[(size_t)k] != P.sc[(size_t)k]) fprintf(stderr, "  scalar %d: %llu, wanted %llu\n", k, (unsigned long long)G.sc[(size_t)k], (unsigned long long)P.sc[(size_t)k]);
			return G.cov;
		};
		for (uint32_t k = 0; k < n_chunks; ++k) {
			uint32_t cid = 0;
			if (ssg_recs_append(r, chunk[k].data(), chunk[k].size(), &cid)) { EXPECT(0, "append: %s", ssg_err_msg.c_str()); return 1; }
			std::vector<uint64_t> hint;
			for (size_t i = 0; i < starts[k].size(); ++i) if (i == 0 || rnd() % 3 == 0) hint.push_back(starts[k][i]);
			if (hint.empty()) hint.push_back(0);
			hint.push_back(chunk[k].size());
			uint64_t n_rec = 0, desc = 0, w_rec = 0, w_desc = 0;
			const int want = plain_push(chunk[k], flt, P, w_rec, w_desc);
			const int rc = ssg_stats_push(st, cid, hint.data(), (int64_t)hint.size() - 1, 0, &n_rec, &desc);
			EXPECT(rc == want && (rc || (n_rec == w_rec && desc == w_desc)), "case %d chunk %u: rc %d (%s), %llu records, %llu descents; wanted %d, %llu, %llu", c, k, rc, ssg_err_msg.c_str(), (unsigned long long)n_rec, (unsigned long long)desc, want, (unsigned long long)w_rec, (unsigned long long)w_desc);
			EXPECT(ssg_stats_push(st, cid + 7, hint.data(), (int64_t)hint.size() - 1, 0, &n_rec, &desc) == SSG_EINVAL && ssg_stats_push(st, cid, hint.data(), (int64_t)hint.size() - 1, 0, 0, 0) == SSG_EINVAL, "a chunk that does not exist, or no place for the numbers");
			++n_push; n_refused += want != 0;
			same(want ? "behind a refused push" : "behind a push");
		}
		EXPECT(ssg_stats_finish(st) == 0, "case %d: finish: %s", c, ssg_err_msg.c_str());
		{ uint64_t a, b; EXPECT(ssg_stats_finish(st) == SSG_EINVAL && ssg_stats_push(st, 0, 0, 0, 0, &a, &b) == SSG_EINVAL, "finish twice, or a push behind it"); }
		plain_finish(P);
		const std::vector<uint64_t> cov = same("behind finish");
		EXPECT(cov == P.cov, "case %d (span %d, max_len %d, %u chunks, sorted %d): the coverage bins differ", c, o.span, o.max_len, n_chunks, (int)P.sc[SSG_ST_SORTED]);
		n_unsorted += !P.sc[SSG_ST_SORTED]; n_bases += P.sc[SSG_ST_TOTAL_LEN];
		ssg_stats_free(st);
		ssg_recs_free(r);
	}
	printf("stats_fuzz: 3000 cases: %ld pushes, %ld of them refused, %ld streams unsorted, %llu bases counted; %ld failures\n", n_push, n_refused, n_unsorted, (unsigned long long)n_bases, n_fail);
	return n_fail ? 1 : 0;
}
