/*
 * b2f_fuzz.cpp -- memory safety and exactness of ssg_b2f_push (k_b2f.h) on the host emulation and under the sanitizers (never on a GPU: a stand-alone program,
 * `make fuzz-b2f` builds and runs it).  3000 seeded cases: a stream of BAM-shaped records over a handful of names, cut into one to three chunks that are each
 * exactly as long as their records plus the store's 16 bytes of slack (heap blocks of the emulation: the sanitizer sees a load behind one).  The records carry
 * what the walks must survive: aux areas of random tags that end in the middle of a tag, of a Z without its NUL, of a B array's header or body, an l_qname of 0
 * and of 255, an l_seq of 0, hard clips, every flag combination -- and, in every fifth case, one record whose l_seq runs its sequence or its qualities past
 * the record's end, by one byte or by many.  A plain C++ restatement of the contract (one map of waiting halves, strings) says what must come back: every push
 * is either SSG_EIO, exactly when its chunk holds such a record and then with the object untouched, or text, counts and the waiting halves equal to the
 * restatement's, with a read group list, with -n and at every hash width.  The sanitizers watch the rest.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <set>
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

static const char *const GROUPS[] = { "g1", "g2", "g", "longer_group" };

static void aux_area(bytes_t &s)
{
	const uint32_t n = rnd() % 5;
	for (uint32_t t = 0; t < n; ++t) {
		const uint32_t kind = rnd() % 12;
		if (kind < 4) { s.push_back('R'); s.push_back('G'); s.push_back('Z'); const char *g = GROUPS[rnd() % 4]; s.insert(s.end(), g, g + strlen(g) + 1); }
		else if (kind == 4) { s.push_back('X'); s.push_back('Z'); s.push_back(rnd() & 1 ? 'Z' : 'H'); for (uint32_t i = rnd() % 6; i > 0; --i) s.push_back('a' + rnd() % 26); if (rnd() % 3) s.push_back(0); }
		else if (kind == 5) { s.push_back('X'); s.push_back('B'); s.push_back('B'); s.push_back("cCsSiIf?"[rnd() % 8]); const uint32_t cnt = rnd() % 4 == 0 ? rnd() : rnd() % 5; s.insert(s.end(), (const uint8_t*)&cnt, (const uint8_t*)&cnt + 4); for (uint32_t i = rnd() % 12; i > 0; --i) s.push_back((uint8_t)rnd()); }
		else if (kind == 6) { s.push_back('X'); s.push_back('D'); s.push_back(rnd() & 1 ? 'd' : (uint8_t)rnd()); for (uint32_t i = rnd() % 9; i > 0; --i) s.push_back((uint8_t)rnd()); }
		else { s.push_back('N'); s.push_back('M'); const char ty = "AcCsSiIf"[rnd() % 8]; s.push_back((uint8_t)ty); const uint32_t sz = ty == 'A' || ty == 'c' || ty == 'C' ? 1 : ty == 's' || ty == 'S' ? 2 : 4; for (uint32_t i = 0; i < sz; ++i) s.push_back((uint8_t)rnd()); }
	}
	if (rnd() % 4 == 0) for (uint32_t i = rnd() % 4; i > 0; --i) s.push_back("RGZXB"[rnd() % 5]);   /* a tag that the record's end cuts */
}

static void record(bytes_t &s, uint32_t n_names)
{
	const uint32_t shape = rnd() % 16;
	const uint32_t l_qname = shape == 0 ? 0 : shape == 1 ? 255 : 2 + rnd() % 3, nc = rnd() % 4, l_seq = rnd() % 5 == 0 ? 0 : rnd() % 70;
	const uint32_t flag = (rnd() % 8 ? 1u : 0u) | (rnd() & 1 ? 0x10u : 0u) | (rnd() & 1 ? 0x40u : 0x80u) | (rnd() % 10 == 0 ? 0x100u : 0u) | (rnd() % 10 == 0 ? 0x800u : 0u) | (rnd() % 6 == 0 ? 0x4u : 0u);
	bytes_t body;
	for (uint32_t i = 0; i + 1 < l_qname; ++i) body.push_back(i == 0 ? (uint8_t)('a' + rnd() % n_names) : l_qname == 255 ? 'L' : 'q');
	if (l_qname) body.push_back(0);
	for (uint32_t i = 0; i < nc; ++i) { const uint32_t v = (1 + rnd() % 90) << 4 | (rnd() % 12 == 0 ? 5u : rnd() % 5); body.insert(body.end(), (const uint8_t*)&v, (const uint8_t*)&v + 4); }
	for (uint32_t i = 0; i < (l_seq + 1) / 2; ++i) body.push_back((uint8_t)rnd());
	for (uint32_t i = 0; i < l_seq; ++i) body.push_back(i == 0 && rnd() % 9 == 0 ? 0xff : (uint8_t)(rnd() % 94));
	aux_area(body);
	const uint32_t core[9] = { 32 + (uint32_t)body.size(), 0, rnd() % 3000u, l_qname | 30u << 8, flag << 16 | nc, l_seq, 0xffffffffu, 0xffffffffu, 0 };
	s.insert(s.end(), (const uint8_t*)core, (const uint8_t*)core + 36);
	s.insert(s.end(), body.begin(), body.end());
}

/* ---- the contract in plain C++ ---- */
struct half_t { std::string seq, qual, rg; bool first; uint64_t size; };
static bool decode(const uint8_t *rec, half_t &h, std::string &name, uint32_t &flag, bool &hard)
{
	uint32_t x[6]; memcpy(x, rec, 24);
	const uint64_t bs = x[0], l_qname = x[3] & 0xff, nc = x[4] & 0xffff, l = x[5];
	flag = x[4] >> 16;
	if (32 + l_qname + 4 * nc + (l + 1) / 2 + l > bs) return false;
	const uint8_t *p = rec + 4 + 32;
	name.assign((const char*)p, l_qname ? l_qname - 1 : 0);
	p += l_qname; hard = false;
	for (uint64_t i = 0; i < nc; ++i) { uint32_t v; memcpy(&v, p + 4 * i, 4); if ((v & 15) == 5) hard = true; }
	p += 4 * nc;
	h.seq.clear(); h.qual.clear();
	for (uint64_t i = 0; i < l; ++i) h.seq += "=ACMGRSVTWYHKDBN"[(p[i >> 1] >> (i & 1 ? 0 : 4)) & 15];
	p += (l + 1) / 2;
	for (uint64_t i = 0; i < l; ++i) h.qual += l > 0 && p[0] == 0xff ? 'I' : (char)(p[i] + 33);
	p += l;
	if (flag & 0x10) {
		std::reverse(h.seq.begin(), h.seq.end()); std::reverse(h.qual.begin(), h.qual.end());
		const char *from = "ACGTMKRYVBHD", *to = "TGCAKMYRBVDH";
		for (char &c : h.seq) { const char *q = strchr(from, c); if (q && c) c = to[q - from]; }
	}
	h.first = (flag & 0x40) != 0; h.rg.clear(); h.size = 4 + bs;
	const uint8_t *e = rec + 4 + bs;
	while (e - p >= 3) {
		const uint8_t t0 = p[0], t1 = p[1], ty = p[2]; p += 3;
		uint64_t sz;
		if (ty == 'A' || ty == 'c' || ty == 'C') sz = 1; else if (ty == 's' || ty == 'S') sz = 2; else if (ty == 'i' || ty == 'I' || ty == 'f') sz = 4;
		else if (ty == 'Z' || ty == 'H') { const uint8_t *q = (const uint8_t*)memchr(p, 0, (size_t)(e - p)); if (!q) break; if (t0 == 'R' && t1 == 'G' && ty == 'Z') h.rg.assign((const char*)p, (size_t)(q - p)); sz = (uint64_t)(q - p) + 1; }
		else if (ty == 'B') { if (e - p < 5) break; uint32_t cnt; memcpy(&cnt, p + 1, 4); sz = 5 + (uint64_t)(p[0] == 'c' || p[0] == 'C' ? 1 : p[0] == 's' || p[0] == 'S' ? 2 : 4) * cnt; }
		else break;
		if (sz > (uint64_t)(e - p)) break;
		p += sz;
	}
	return true;
}
struct plain_t {
	std::set<std::string> want; bool rename; uint64_t counter; std::map<std::string, half_t> waiting;
	/* false: a malformed record, nothing changes */
	bool push(const bytes_t &s, std::string &out, uint64_t &n_rec, uint64_t &n_pairs)
	{
		out.clear(); n_rec = n_pairs = 0;
		half_t h; std::string name; uint32_t flag; bool hard;
		for (uint64_t o = 0; o < s.size(); ) { uint32_t bs; memcpy(&bs, s.data() + o, 4); if (!decode(s.data() + o, h, name, flag, hard)) return false; o += 4 + (uint64_t)bs; }
		for (uint64_t o = 0; o < s.size(); ) {
			uint32_t bs; memcpy(&bs, s.data() + o, 4);
			decode(s.data() + o, h, name, flag, hard);
			o += 4 + (uint64_t)bs; ++n_rec;
			if ((flag & 0x900) || hard || !(flag & 1)) continue;
			if (!want.empty() && !want.count(h.rg)) continue;
			auto it = waiting.find(name);
			if (it == waiting.end()) { waiting[name] = h; continue; }
			if (it->second.first == h.first) continue;
			const half_t &a = h.first ? h : it->second, &b = h.first ? it->second : h;
			const std::string nm = rename ? std::to_string(counter) : name;
			out += "@" + nm + "/1" + (a.rg.empty() ? "" : " RG:Z:" + a.rg) + "\n" + a.seq + "\n+\n" + a.qual + "\n";
			out += "@" + nm + "/2" + (b.rg.empty() ? "" : " RG:Z:" + b.rg) + "\n" + b.seq + "\n+\n" + b.qual + "\n";
			++counter; ++n_pairs;
			waiting.erase(it);
		}
		return true;
	}
};

int main()
{
	long n_eio = 0, n_text = 0; uint64_t n_pairs_all = 0;
	for (int c = 0; c < 3000; ++c) {
		rng_s = 0x9e3779b97f4a7c15ull ^ ((uint64_t)(c + 1) * 0x2545f4914f6cdd1dull);
		const uint32_t n_chunks = 1 + rnd() % 3, n_names = 1 + rnd() % 6;
		plain_t P; P.rename = rnd() % 3 == 0; P.counter = 0;
		std::vector<const char*> ids;
		if (rnd() % 3 == 0) for (uint32_t g = 1 + rnd() % 2; g > 0; --g) { ids.push_back(GROUPS[rnd() % 4]); P.want.insert(ids.back()); }
		static const int BITS[] = { 64, 64, 7, 1, 0 };
		ssg_recs_t *r = 0; ssg_b2f_t *b = 0;
		if (ssg_recs_create(~(uint64_t)0 >> 1, &r) || ssg_b2f_create(r, ids.empty() ? 0 : ids.data(), (int)ids.size(), P.rename, BITS[rnd() % 5], &b)) { EXPECT(0, "create: %s", ssg_err_msg.c_str()); return 1; }
		for (uint32_t k = 0; k < n_chunks; ++k) {
			bytes_t s; std::vector<uint64_t> starts;
			const uint32_t n = rnd() % 60;
			for (uint32_t i = 0; i < n; ++i) { starts.push_back(s.size()); record(s, n_names); }
			if (n && c % 5 == 0 && rnd() % 2) {   /* a sequence that leaves its record */
				const uint64_t o = starts[rnd() % n]; uint32_t x[6]; memcpy(x, s.data() + o, 24);
				const uint64_t room = x[0] - 32 - (x[3] & 0xff) - 4 * (uint64_t)(x[4] & 0xffff);   /* bytes behind the CIGAR */
				uint32_t l = 0; while (((uint64_t)l + 1) / 2 + l <= room) ++l;                     /* the smallest l_seq that does not fit */
				if (rnd() % 3 == 0) l = rnd() % 2 ? 0x7fffffffu : 0xffffffffu; else l += rnd() % 2 ? 0 : rnd() % 50;
				memcpy(s.data() + o + 20, &l, 4);
			}
			std::vector<uint64_t> hint;
			for (size_t i = 0; i < starts.size(); ++i) if (i == 0 || rnd() % 3 == 0) hint.push_back(starts[i]);
			if (hint.empty()) hint.push_back(0);
			hint.push_back(s.size());
			uint32_t cid = 0;
			if (ssg_recs_append(r, s.data(), s.size(), &cid)) { EXPECT(0, "append: %s", ssg_err_msg.c_str()); return 1; }
			uint64_t held0 = 0, bytes0 = 0, held1 = 0, bytes1 = 0; ssg_b2f_waiting(b, &held0, &bytes0);
			std::string want; uint64_t w_rec = 0, w_pairs = 0;
			const bool good = P.push(s, want, w_rec, w_pairs);
			const uint64_t cap = 2 * (s.size() + bytes0) + 64;
			bytes_t out((size_t)cap);   /* exactly the documented bound: a byte more is the sanitizer's */
			uint64_t out_len = 0, n_rec = 0, n_pairs = 0;
			const int rc = ssg_b2f_push(b, cid, hint.data(), (int64_t)hint.size() - 1, 0, out.data(), cap, &out_len, &n_rec, &n_pairs);
			ssg_b2f_waiting(b, &held1, &bytes1);
			if (!good) {
				++n_eio;
				EXPECT(rc == SSG_EIO && ssg_err_msg.find("l_seq") != std::string::npos, "case %d chunk %u: rc %d (%s), a malformed record is in the chunk", c, k, rc, ssg_err_msg.c_str());
				EXPECT(held1 == held0 && bytes1 == bytes0 && n_pairs == 0, "case %d chunk %u: the object changed on a failure", c, k);
				EXPECT(ssg_recs_release(r, cid) == 0, "case %d chunk %u: the chunk is gone after a failure", c, k);
				continue;
			}
			++n_text; n_pairs_all += w_pairs;
			EXPECT(rc == 0, "case %d chunk %u: rc %d (%s)", c, k, rc, ssg_err_msg.c_str());
			if (rc) break;
			uint64_t w_bytes = 0; for (const auto &kv : P.waiting) w_bytes += kv.second.size;
			EXPECT(n_rec == w_rec && n_pairs == w_pairs && out_len == want.size() && !memcmp(out.data(), want.data(), want.size()), "case %d chunk %u: %llu records, %llu pairs, %llu bytes; wanted %llu, %llu, %zu (or other text)",
			       c, k, (unsigned long long)n_rec, (unsigned long long)n_pairs, (unsigned long long)out_len, (unsigned long long)w_rec, (unsigned long long)w_pairs, want.size());
			EXPECT(held1 == P.waiting.size() && bytes1 == w_bytes, "case %d chunk %u: %llu halves of %llu bytes wait, wanted %zu of %llu", c, k, (unsigned long long)held1, (unsigned long long)bytes1, P.waiting.size(), (unsigned long long)w_bytes);
		}
		ssg_b2f_free(b);
		ssg_recs_free(r);
	}
	printf("b2f_fuzz: 3000 cases: %ld pushes gave text (%llu pairs), %ld were SSG_EIO; %ld failures\n", n_text, (unsigned long long)n_pairs_all, n_eio, n_fail);
	return n_fail ? 1 : 0;
}
