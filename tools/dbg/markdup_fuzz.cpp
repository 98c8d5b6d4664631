/*
 * markdup_fuzz.cpp -- memory safety and exactness of ssg_markdup_* (k_markdup.h) on the host emulation and under the sanitizers (never on a GPU: a stand-alone
 * program, `make fuzz-markdup` builds and runs it).  3000 seeded cases: a stream of BAM-shaped records -- every flag bit, CIGARs of every operation code with
 * clips at either end, in the middle and alone, an l_seq of 0, qualities of every byte, names that come twice, three and four times, with and without NUL, aux
 * areas of every type that end where they should, are cut short or are noise, with RG:Z values inside and outside the list -- at a handful of positions so that
 * groups form, in one to three chunks, each exactly as long as its records plus the store's 16 bytes of slack (a heap block of the emulation: the sanitizer sees a
 * load behind it); every hash width from 0 to 64 bits.  In every seventh case one record is broken (an l_seq that leaves the record): the push is SSG_EIO and the
 * object as before.  A plain C++ loop of the rule (std::map keyed by tuples, names as strings, nothing hashed) says which ordinals are duplicates and what the
 * eight counts are; the second pass is held to the input's bytes under a mask of the one bit, with and without `remove'.  One case carries a record of 5 M
 * qualities of 0xff: the score saturates at 2^30 - 1.  Every refusal of the arguments and of the state is asked for once a case.  The sanitizers watch the rest.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <set>
#include <string>
#include <tuple>
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

static const char *const RG[4] = { "a", "bb", "a1", "lib" };
static const uint16_t LIB[4] = { 1, 2, 1, 0 };

static void put32(bytes_t &b, uint32_t v) { b.insert(b.end(), (const uint8_t*)&v, (const uint8_t*)&v + 4); }
static void aux_area(bytes_t &b)
{
	const uint32_t kind = rnd() % 8;
	if (kind == 0) return;
	if (kind == 1) { for (uint32_t i = rnd() % 12; i > 0; --i) b.push_back((uint8_t)rnd()); return; }   /* noise */
	for (uint32_t n = 1 + rnd() % 4; n > 0; --n) {
		const bool rg = rnd() % 2 == 0;
		b.push_back(rg ? 'R' : 'X'); b.push_back(rg ? 'G' : (uint8_t)('a' + rnd() % 26));
		static const char types[] = "AcCsSiIfZHBd";
		const char ty = rg && rnd() % 6 ? 'Z' : types[rnd() % 12];
		b.push_back((uint8_t)ty);
		uint32_t sz = ty == 'A' || ty == 'c' || ty == 'C' ? 1 : ty == 's' || ty == 'S' ? 2 : ty == 'd' ? 8 : 4;
		if (ty == 'Z' || ty == 'H') {
			if (rg && rnd() % 4) { const char *g = RG[rnd() % 4]; b.insert(b.end(), g, g + strlen(g)); if (rnd() % 8 == 0) b.push_back('x'); }
			else for (uint32_t i = rnd() % 4; i > 0; --i) b.push_back((uint8_t)('a' + rnd() % 3));
			if (rnd() % 10) b.push_back(0);
			continue;
		}
		if (ty == 'B') { const char st = "cCsSiIf"[rnd() % 7]; const uint32_t cnt = rnd() % 4; b.push_back((uint8_t)st); put32(b, rnd() % 30 == 0 ? 0xffffffffu : cnt); sz = cnt * (st == 'c' || st == 'C' ? 1 : st == 's' || st == 'S' ? 2 : 4); }
		if (rnd() % 12 == 0 && sz) sz = rnd() % sz;   /* cut short */
		for (uint32_t i = 0; i < sz; ++i) b.push_back((uint8_t)rnd());
	}
}
static void record(bytes_t &s, uint32_t n_names, uint32_t l_seq_big)
{
	char nm[16]; const int nl = snprintf(nm, sizeof(nm), "q%u", rnd() % n_names);
	const uint32_t l_qname = rnd() % 40 == 0 ? 0 : (uint32_t)nl + 1, nc = l_seq_big ? 1 : rnd() % 12 == 0 ? 0 : 1 + rnd() % 5;
	uint32_t flag = 0;
	static const uint32_t bits[12] = { 1, 2, 4, 8, 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x400, 0x800 }; static const uint32_t odds[12] = { 2, 2, 14, 12, 2, 2, 2, 2, 14, 8, 6, 14 };
	for (int k = 0; k < 12; ++k) if (rnd() % odds[k] == 0) flag |= bits[k];
	if (l_seq_big) flag &= 0x10;   /* (the long records take part) */
	bytes_t body;
	for (uint32_t i = 0; i < l_qname; ++i) body.push_back(i + 1 == l_qname && rnd() % 8 ? 0 : (uint8_t)nm[i < (uint32_t)nl ? i : 0]);
	for (uint32_t i = 0; i < nc; ++i) {
		const uint32_t op = rnd() % 16 == 0 ? 9 + rnd() % 7 : rnd() % 2 == 0 ? 4 + rnd() % 2 : rnd() % 9, len = rnd() % 12 == 0 ? 0 : (op == 4 || op == 5) && rnd() % 20 == 0 ? 0xfffffffu : 1 + rnd() % 4;   /* (a long clip: u5 beyond 32 bits; the scan's `end' is not this program's subject) */
		put32(body, len << 4 | op);
	}
	const uint32_t l_seq = l_seq_big ? l_seq_big : rnd() % 8 == 0 ? 0 : rnd() % 6 == 0 ? 60 + rnd() % 80 : 1 + rnd() % 9;
	for (uint32_t i = 0; i < (l_seq + 1) / 2; ++i) body.push_back((uint8_t)rnd());
	const uint32_t qk = l_seq_big ? 0 : rnd() % 4;
	for (uint32_t i = 0; i < l_seq; ++i) body.push_back(qk == 0 ? 0xff : qk == 1 ? (uint8_t)rnd() : qk == 2 ? (uint8_t)(13 + rnd() % 4) : 30);
	aux_area(body);
	const int32_t tid = rnd() % 20 == 0 ? -1 : (int32_t)(rnd() % 2), pos = rnd() % 30 == 0 ? 0x7fffff00 : rnd() % 30 == 0 ? -1 : (int32_t)(rnd() % 6);
	const uint32_t core[9] = { 32 + (uint32_t)body.size(), (uint32_t)tid, (uint32_t)pos, l_qname | 30u << 8, flag << 16 | nc, l_seq, (uint32_t)tid, (uint32_t)pos, 0 };
	s.insert(s.end(), (const uint8_t*)core, (const uint8_t*)core + 36);
	s.insert(s.end(), body.begin(), body.end());
}

/* ---- the rule in plain C++ ---- */
typedef std::tuple<uint32_t, int32_t, int64_t, int> end_key_t;   /* library, tid, u5, rev */
struct fact_t { bool good, taking, paired; end_key_t key; uint32_t score, flag, bs; std::string name; };
static fact_t fact_of(const uint8_t *rec)
{
	uint32_t x[6]; memcpy(x, rec, 24);
	const uint32_t bs = x[0], lq = x[3] & 0xff, nc = x[4] & 0xffff, flag = x[4] >> 16, l = x[5];
	fact_t f; f.bs = bs; f.flag = flag; f.taking = f.paired = false; f.score = 0;
	uint64_t a = 32 + (uint64_t)lq + 4 * (uint64_t)nc + ((uint64_t)l + 1) / 2 + l;
	f.good = a <= bs;
	if (!f.good) return f;
	const uint8_t *body = rec + 4;
	f.name.assign((const char*)body + 32, lq ? lq - 1 : 0);
	f.taking = !(flag & 0x904) && nc > 0;
	if (!f.taking) return f;
	std::vector<std::pair<uint32_t, int64_t> > ops;
	for (uint32_t k = 0; k < nc; ++k) { uint32_t c; memcpy(&c, body + 32 + lq + 4 * k, 4); ops.push_back(std::make_pair(c & 15u, (int64_t)(c >> 4))); }
	int64_t lead = 0, trail = 0, span = 0;
	for (size_t k = 0; k < ops.size() && (ops[k].first == 4 || ops[k].first == 5); ++k) lead += ops[k].second;
	for (size_t k = ops.size(); k > 0 && (ops[k - 1].first == 4 || ops[k - 1].first == 5); --k) trail += ops[k - 1].second;
	for (const auto &o : ops) if (o.first == 0 || o.first == 2 || o.first == 3 || o.first == 7 || o.first == 8) span += o.second;
	const int rev = flag >> 4 & 1; const int64_t pos = (int32_t)x[2];
	uint64_t sum = 0;
	const uint8_t *q = body + 32 + lq + 4 * nc + (l + 1) / 2;
	for (uint32_t i = 0; i < l; ++i) if (q[i] >= 15) sum += q[i];
	f.score = (uint32_t)std::min<uint64_t>(sum, (1u << 30) - 1);
	/* the last RG:Z of the aux area */
	std::string rg; bool have = false;
	const uint64_t e = bs;
	while (a + 3 <= e) {
		const uint8_t t0 = body[a], t1 = body[a + 1], ty = body[a + 2];
		a += 3;
		if (ty == 'A' || ty == 'c' || ty == 'C') a += 1;
		else if (ty == 's' || ty == 'S') a += 2;
		else if (ty == 'i' || ty == 'I' || ty == 'f') a += 4;
		else if (ty == 'Z' || ty == 'H') {
			uint64_t z = a; while (z < e && body[z]) ++z;
			if (z >= e) break;
			if (t0 == 'R' && t1 == 'G' && ty == 'Z') { rg.assign((const char*)body + a, (size_t)(z - a)); have = true; }
			a = z + 1;
		} else if (ty == 'B') {
			if (a + 5 > e) break;
			uint32_t cnt; memcpy(&cnt, body + a + 1, 4);
			const uint8_t st = body[a];
			a += 5 + (uint64_t)((st == 'c' || st == 'C') ? 1 : (st == 's' || st == 'S') ? 2 : 4) * cnt;
		} else break;
	}
	uint32_t lib = 0;
	if (have) for (int g = 3; g >= 0; --g) if (rg == RG[g]) lib = LIB[g];
	f.key = end_key_t(lib, (int32_t)x[1], rev ? pos + span - 1 + trail : pos - lead, rev);
	f.paired = (flag & 1) && !(flag & 8);
	return f;
}
struct plain_t { std::vector<fact_t> f; };
static void plain_decide(const plain_t &P, std::set<uint64_t> &dup, uint64_t *c)
{
	for (int k = 0; k < SSG_MD_N; ++k) c[k] = 0;
	const std::vector<fact_t> &f = P.f;
	std::map<std::string, uint64_t> held; std::vector<std::pair<uint64_t, uint64_t> > pairs;
	for (uint64_t o = 0; o < f.size(); ++o) {
		++c[SSG_MD_RECORDS];
		if (!f[o].taking) continue;
		++c[SSG_MD_TAKING_PART];
		if (!f[o].paired) { ++c[SSG_MD_FRAGMENTS]; continue; }
		++c[SSG_MD_PAIRED];
		auto h = held.find(f[o].name);
		if (h == held.end()) held[f[o].name] = o;
		else if ((f[h->second].flag & 0xc0) == (f[o].flag & 0xc0)) {}
		else { pairs.push_back(std::make_pair(h->second, o)); held.erase(h); }
	}
	c[SSG_MD_PAIRS] = pairs.size(); c[SSG_MD_UNMATCHED] = c[SSG_MD_PAIRED] - 2 * pairs.size();
	auto order = [](const end_key_t &k) { return std::make_tuple(std::get<1>(k), std::get<2>(k), std::get<3>(k), std::get<0>(k)); };
	std::map<std::pair<end_key_t, end_key_t>, std::vector<std::pair<uint64_t, uint64_t> > > groups;
	for (const auto &p : pairs) {
		const end_key_t &a = f[p.first].key, &b = f[p.second].key;
		groups[order(a) <= order(b) ? std::make_pair(a, b) : std::make_pair(b, a)].push_back(p);
	}
	for (const auto &g : groups) {
		uint64_t best = 0, best_score = 0; bool any = false;
		for (const auto &p : g.second) { const uint64_t s = (uint64_t)f[p.first].score + f[p.second].score; if (!any || s > best_score) { best = p.first; best_score = s; any = true; } }   /* (pairs are listed by their later record; the pair ordinal is the earlier one) */
		for (const auto &p : g.second) { const uint64_t s = (uint64_t)f[p.first].score + f[p.second].score; if (s == best_score && p.first < best) best = p.first; }
		for (const auto &p : g.second) if (p.first != best) { dup.insert(p.first); dup.insert(p.second); c[SSG_MD_DUP_PAIRED] += 2; }
	}
	std::map<end_key_t, std::vector<uint64_t> > ends;
	for (uint64_t o = 0; o < f.size(); ++o) if (f[o].taking) ends[f[o].key].push_back(o);
	for (const auto &g : ends) {
		bool any_paired = false; uint64_t keep = ~(uint64_t)0;
		for (uint64_t o : g.second) any_paired = any_paired || f[o].paired;
		if (!any_paired) for (uint64_t o : g.second) if (keep == ~(uint64_t)0 || f[o].score > f[keep].score) keep = o;
		for (uint64_t o : g.second) if (!f[o].paired && o != keep) { dup.insert(o); ++c[SSG_MD_DUP_FRAGMENTS]; }
	}
}

int main()
{
	long n_push = 0, n_refused = 0; uint64_t n_dup = 0, n_recs = 0, n_range = 0;
	const char *rg_null[2] = { "a", 0 }, *rg_empty[2] = { "a", "" };
	for (int c = 0; c < 3000; ++c) {
		rng_s = 0x9e3779b97f4a7c15ull ^ ((uint64_t)(c + 1) * 0x2545f4914f6cdd1dull);
		const bool wide = c % 50 == 3;   /* one run of the join, longer than the limit where more than 256 records are paired */
		const int hash_bits = wide ? 0 : c % 4 == 0 ? 64 : (int)(rnd() % 65);
		const uint32_t n = c == 7 ? 3 : wide ? 500 + rnd() % 600 : rnd() % 200, n_chunks = 1 + rnd() % 3, n_names = 1 + rnd() % (n + 1);
		const bool with_rg = rnd() % 4 != 0;
		std::vector<bytes_t> chunk(n_chunks); std::vector<std::vector<uint64_t> > starts(n_chunks);
		for (uint32_t i = 0; i < n; ++i) { const uint32_t k = (uint32_t)((uint64_t)i * n_chunks / n); starts[k].push_back(chunk[k].size()); record(chunk[k], n_names, c == 7 && i < 2 ? 5000000 + i : 0); }
		int broken = -1;
		if (c % 7 == 0 && c != 7 && n > 0) {   /* one broken record */
			uint32_t k = rnd() % n_chunks; while (starts[k].empty()) k = (k + 1) % n_chunks;
			bytes_t &s = chunk[k]; const uint64_t ro = starts[k][rnd() % starts[k].size()]; uint32_t x[6]; memcpy(x, s.data() + ro, 24);
			const uint32_t l = rnd() % 2 ? 0x7fffffffu : x[5] + 1 + rnd() % 60 + 2 * (x[0] - 32); memcpy(s.data() + ro + 20, &l, 4);
			broken = (int)k;
		}
		ssg_recs_t *r = 0; ssg_markdup_t *m = 0;
		if (ssg_recs_create(~(uint64_t)0 >> 1, &r)) { EXPECT(0, "create: %s", ssg_err_msg.c_str()); return 1; }
		{	/* what create refuses */
			ssg_markdup_t *x = 0;
			EXPECT(ssg_markdup_create(0, RG, LIB, 4, 64, &x) == SSG_EINVAL && ssg_markdup_create(r, rg_null, LIB, 2, 64, &x) == SSG_EINVAL && ssg_markdup_create(r, rg_empty, LIB, 2, 64, &x) == SSG_EINVAL
			       && ssg_markdup_create(r, RG, LIB, -1, 64, &x) == SSG_EINVAL && ssg_markdup_create(r, RG, LIB, 4, -1, &x) == SSG_EINVAL && ssg_markdup_create(r, RG, LIB, 4, 65, &x) == SSG_EINVAL
			       && ssg_markdup_create(r, RG, 0, 4, 64, &x) == SSG_EINVAL && ssg_markdup_create(r, RG, LIB, 4, 64, 0) == SSG_EINVAL, "a bad store, id, count, hash width or no handle was taken");
		}
		if (ssg_markdup_create(r, with_rg ? RG : 0, with_rg ? LIB : 0, with_rg ? 4 : 0, hash_bits, &m)) { EXPECT(0, "create: %s", ssg_err_msg.c_str()); return 1; }
		plain_t P; std::vector<bytes_t> pushed;
		for (uint32_t k = 0; k < n_chunks; ++k) {
			uint32_t cid = 0;
			if (ssg_recs_append(r, chunk[k].data(), chunk[k].size(), &cid)) { EXPECT(0, "append: %s", ssg_err_msg.c_str()); return 1; }
			std::vector<uint64_t> hint;
			for (size_t i = 0; i < starts[k].size(); ++i) if (i == 0 || rnd() % 3 == 0) hint.push_back(starts[k][i]);
			if (hint.empty()) hint.push_back(0);
			hint.push_back(chunk[k].size());
			uint64_t n_rec = 0, dummy = 0; uint8_t d1 = 0;
			EXPECT(ssg_markdup_push(m, cid + 7, hint.data(), (int64_t)hint.size() - 1, 0, &n_rec) == SSG_EINVAL && ssg_markdup_push(m, cid, hint.data(), (int64_t)hint.size() - 1, 0, 0) == SSG_EINVAL
			       && ssg_markdup_get(m, 0, 0, &d1) == SSG_EINVAL && ssg_markdup_apply(m, cid, hint.data(), (int64_t)hint.size() - 1, 0, 0, 0, &n_rec, &dummy, 0, 0) == SSG_EINVAL,
			       "a chunk that does not exist, no place for the number, or get / apply before finish");
			const int want = (int)k == broken ? SSG_EIO : 0;
			const int rc = ssg_markdup_push(m, cid, hint.data(), (int64_t)hint.size() - 1, 0, &n_rec);
			EXPECT(rc == want && (rc || n_rec == starts[k].size()), "case %d chunk %u: rc %d (%s), %llu records; wanted %d, %zu", c, k, rc, ssg_err_msg.c_str(), (unsigned long long)n_rec, want, starts[k].size());
			++n_push; n_refused += want != 0;
			if (rc) { if (ssg_recs_release(r, cid)) EXPECT(0, "a refused push released its chunk"); continue; }
			for (uint64_t ro : starts[k]) { fact_t f = fact_of(chunk[k].data() + ro); if (with_rg == false) std::get<0>(f.key) = 0; P.f.push_back(f); }
			pushed.push_back(chunk[k]);
		}
		std::set<uint64_t> dup; uint64_t want_c[SSG_MD_N], got_c[SSG_MD_N + 1]; got_c[SSG_MD_N] = 0xabab;
		plain_decide(P, dup, want_c);
		const int frc = ssg_markdup_finish(m, got_c);
		if (hash_bits == 0 && want_c[SSG_MD_PAIRED] > SSG_MARKDUP_RUN_MAX) {   /* every paired record in one run */
			uint8_t d1 = 0;
			EXPECT(frc == SSG_ERANGE && ssg_markdup_get(m, 0, 0, &d1) == SSG_EINVAL, "case %d: %llu paired records in one run: rc %d", c, (unsigned long long)want_c[SSG_MD_PAIRED], frc);
			++n_range; ssg_markdup_free(m); ssg_recs_free(r); continue;
		}
		EXPECT(frc == 0 && got_c[SSG_MD_N] == 0xabab && !memcmp(got_c, want_c, sizeof(want_c)), "case %d (hash_bits %d, %u records): finish rc %d (%s); counts %llu %llu %llu %llu %llu %llu %llu %llu, wanted %llu %llu %llu %llu %llu %llu %llu %llu", c, hash_bits, n, frc, ssg_err_msg.c_str(),
		       (unsigned long long)got_c[0], (unsigned long long)got_c[1], (unsigned long long)got_c[2], (unsigned long long)got_c[3], (unsigned long long)got_c[4], (unsigned long long)got_c[5], (unsigned long long)got_c[6], (unsigned long long)got_c[7],
		       (unsigned long long)want_c[0], (unsigned long long)want_c[1], (unsigned long long)want_c[2], (unsigned long long)want_c[3], (unsigned long long)want_c[4], (unsigned long long)want_c[5], (unsigned long long)want_c[6], (unsigned long long)want_c[7]);
		if (frc) { ssg_markdup_free(m); ssg_recs_free(r); continue; }
		{ uint64_t a; EXPECT(ssg_markdup_finish(m, got_c) == SSG_EINVAL && ssg_markdup_push(m, 0, 0, 0, 0, &a) == SSG_EINVAL, "finish twice, or a push behind it"); }
		const uint64_t N = P.f.size();
		bytes_t bits((size_t)N);   /* exactly as long as the ordinals */
		EXPECT(ssg_markdup_get(m, 0, N, bits.data()) == 0 && ssg_markdup_get(m, 1, N, bits.data()) == SSG_EINVAL, "case %d: get", c);
		size_t n_bad = 0;
		for (uint64_t o = 0; o < N; ++o) n_bad += (bits[(size_t)o] != 0) != (dup.count(o) != 0);
		EXPECT(n_bad == 0, "case %d (hash_bits %d, %llu records): %zu duplicate bits differ", c, hash_bits, (unsigned long long)N, n_bad);
		if (c == 7) EXPECT(N == 3 && P.f[0].score == (1u << 30) - 1 && P.f[1].score == (1u << 30) - 1, "the saturation case does not saturate");
		n_dup += dup.size(); n_recs += N;
		/* the second pass */
		const int remove = (int)(rnd() % 2);
		uint64_t ord = 0;
		for (size_t k = 0; k < pushed.size(); ++k) {
			uint32_t cid = 0;
			if (ssg_recs_append(r, pushed[k].data(), pushed[k].size(), &cid)) { EXPECT(0, "append: %s", ssg_err_msg.c_str()); return 1; }
			const uint64_t hint[2] = { 0, pushed[k].size() };
			uint64_t n_rec = 0, n_kept = 0, c_rec = 0, c_kept = 0;
			const size_t cap = pushed[k].size() / 36 + 1;
			std::vector<uint64_t> loc(cap); std::vector<ssg_bam_ent_t> ent(cap);
			EXPECT(ssg_markdup_apply(m, cid, hint, 1, 0, remove, 0, &c_rec, &c_kept, 0, 0) == 0, "case %d: the counting form: %s", c, ssg_err_msg.c_str());
			const int rc = ssg_markdup_apply(m, cid, hint, 1, 0, remove, cap, &n_rec, &n_kept, loc.data(), ent.data());
			EXPECT(rc == 0 && n_rec == c_rec && n_kept == c_kept, "case %d: apply rc %d (%s)", c, rc, ssg_err_msg.c_str());
			if (rc) break;
			bytes_t want;
			uint64_t o = 0;
			for (uint64_t i = 0; i < n_rec; ++i, ++ord) {
				uint32_t bs; memcpy(&bs, pushed[k].data() + o, 4);
				const bool d = dup.count(ord) != 0;
				if (!(remove && d && P.f[(size_t)ord].taking)) {
					const size_t at = want.size();
					want.insert(want.end(), pushed[k].begin() + (ptrdiff_t)o, pushed[k].begin() + (ptrdiff_t)(o + 4 + bs));
					if (P.f[(size_t)ord].taking) want[at + 19] = (uint8_t)((want[at + 19] & ~4u) | (d ? 4u : 0u));
				}
				o += 4 + (uint64_t)bs;
			}
			std::vector<uint64_t> cum((size_t)n_kept + 1, 0);
			for (uint64_t i = 0; i < n_kept; ++i) cum[(size_t)i + 1] = cum[(size_t)i] + ent[(size_t)i].len;
			bytes_t got((size_t)cum[(size_t)n_kept]);
			EXPECT(cum[(size_t)n_kept] == want.size() && ssg_recs_order(r, loc.data(), cum.data(), (int64_t)n_kept) == 0 && ssg_recs_gather(r, 0, cum[(size_t)n_kept], got.data()) == 0 && got == want,
			       "case %d chunk %zu (remove %d): the bytes behind the second pass differ (%s)", c, k, remove, ssg_err_msg.c_str());
			if (ssg_recs_reopen(r) || ssg_recs_release(r, cid)) EXPECT(0, "reopen / release: %s", ssg_err_msg.c_str());
		}
		ssg_markdup_free(m);
		ssg_recs_free(r);
	}
	printf("markdup_fuzz: 3000 cases: %ld pushes, %ld of them refused, %llu records decided, %llu duplicates, %llu cases past the run limit; %ld failures\n", n_push, n_refused,
	       (unsigned long long)n_recs, (unsigned long long)n_dup, (unsigned long long)n_range, n_fail);
	return n_fail ? 1 : 0;
}
