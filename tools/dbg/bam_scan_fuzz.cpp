/*
 * bam_scan_fuzz.cpp -- memory safety of ssg_recs_scan's walks (k_bam_scan.h) on streams that are not what they should be, on the host emulation and under the
 * sanitizers (never on a GPU: a stand-alone program, `make fuzz-bam-scan` builds and runs it).  A stream of BAM-shaped records goes into a chunk of the store
 * that is exactly as long as the stream plus the store's 16 bytes of slack (a heap block of the emulation: the sanitizer sees a load behind it), with hints at
 * record starts; then 3000 seeded mutations: other block_size words (small, huge, all ones), other l_qname / n_cigar, truncated streams, hints moved into the
 * middle of records.  Checked: the return code is 0, SSG_EIO or SSG_EALIGN; 0 exactly when a plain walk of the stream from `first' is good and every hint that
 * was entered is a record start -- then with that walk's offsets, keys and ends.  The sanitizers watch the rest.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
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

static void record(bytes_t &s)
{
	const uint32_t l_qname = 1 + rnd() % 12, nc = rnd() % 6, l_seq = rnd() % 40, flag = (rnd() & 1 ? 16u : 0u) | (rnd() % 7 == 0 ? 4u : 0u);
	const uint32_t bs = 32 + l_qname + 4 * nc + (l_seq + 1) / 2 + l_seq + rnd() % 9;
	uint32_t core[9] = { bs, (uint32_t)((int32_t)(rnd() % 4) - 1), rnd() % 1000000u, l_qname | 30u << 8, flag << 16 | nc, l_seq, 0xffffffffu, 0xffffffffu, 0 };
	s.insert(s.end(), (uint8_t*)core, (uint8_t*)core + 36);
	for (uint32_t i = 0; i < l_qname; ++i) s.push_back(i + 1 < l_qname ? 'q' : 0);
	for (uint32_t i = 0; i < nc; ++i) { const uint32_t v = (1 + rnd() % 90) << 4 | rnd() % 9; s.insert(s.end(), (uint8_t*)&v, (uint8_t*)&v + 4); }
	const size_t rest = bs - 32 - l_qname - 4 * nc;
	for (size_t i = 0; i < rest; ++i) s.push_back((uint8_t)rnd());
}

struct walk_t { std::vector<uint64_t> off, key; std::vector<int32_t> end; bool good; };
/* the plain walk: good iff the records tile s[first ..) exactly and every one holds its name and CIGAR */
static walk_t plain_walk(const bytes_t &s, uint64_t first)
{
	walk_t w; w.good = true; uint64_t o = first;
	while (o < s.size()) {
		if (o + 4 > s.size()) { w.good = false; break; }
		uint32_t x[5]; memcpy(x, s.data() + o, 4);
		if (x[0] < 32 || (uint64_t)x[0] > s.size() - o - 4) { w.good = false; break; }
		memcpy(x, s.data() + o, 20);
		const uint32_t l_qname = x[3] & 0xff, nc = x[4] & 0xffff, flag = x[4] >> 16;
		if (l_qname + 4 * nc > x[0] - 32) w.good = false;
		int32_t end = (int32_t)x[2] + 1;
		if (w.good && !(flag & 4) && nc) { int32_t rl = 0; for (uint32_t i = 0; i < nc; ++i) { uint32_t v; memcpy(&v, s.data() + o + 36 + l_qname + 4 * i, 4); const uint32_t op = v & 15; if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += (int32_t)(v >> 4); } end = (int32_t)x[2] + rl; }
		w.off.push_back(o); w.end.push_back(end);
		w.key.push_back((uint64_t)(int64_t)(int32_t)x[1] << 32 | (uint64_t)(uint32_t)((x[2] + 1u) << 1) | (flag & 16 ? 1u : 0u));
		o += 4 + (uint64_t)x[0];
	}
	return w;
}

static void judge(const bytes_t &s, const std::vector<uint64_t> &hint, uint64_t first, int it)
{
	ssg_recs_t *r = 0; uint32_t cid = 0;
	if (ssg_recs_create(s.size(), &r) || ssg_recs_append(r, s.data(), s.size(), &cid)) { EXPECT(0, "store: %s", ssg_err_msg.c_str()); return; }
	const size_t cap = s.size() / 36 + 1;
	std::vector<uint64_t> loc(cap), key(cap); std::vector<ssg_bam_ent_t> ent(cap); uint64_t n = 0;
	const int rc = ssg_recs_scan(r, cid, hint.data(), (int64_t)hint.size() - 1, first, cap, &n, loc.data(), key.data(), ent.data());
	ssg_recs_free(r);
	EXPECT(rc == 0 || rc == SSG_EIO || rc == SSG_EALIGN, "%d: rc %d (%s)", it, rc, ssg_err_msg.c_str());
	const walk_t w = plain_walk(s, first);
	bool hints_ok = true;   /* every hint behind `first' and in front of the end is a record start */
	for (size_t b = 0; b + 1 < hint.size(); ++b) if (hint[b] > first && hint[b] < s.size() && !std::binary_search(w.off.begin(), w.off.end(), hint[b])) hints_ok = false;
	const bool want_good = w.good && hints_ok;
	EXPECT((rc == 0) == want_good, "%d: rc %d (%s), the plain walk says %s, the hints %s", it, rc, ssg_err_msg.c_str(), w.good ? "good" : "bad", hints_ok ? "hold" : "do not hold");
	if (rc == 0 && want_good) {
		EXPECT(n == w.off.size(), "%d: %llu records, %zu expected", it, (unsigned long long)n, w.off.size());
		for (size_t i = 0; i < w.off.size() && i < n; ++i)
			EXPECT(loc[i] == ((uint64_t)cid << 40 | w.off[i]) && key[i] == w.key[i] && ent[i].end == w.end[i], "%d: record %zu differs", it, i);
	}
}

int main()
{
	long n_good = 0;
	for (int it = 0; it < 3000; ++it) {
		bytes_t s; std::vector<uint64_t> starts;
		const int n_rec = 1 + (int)(rnd() % 40);
		const uint64_t first = rnd() % 3 == 0 ? 1 + rnd() % 50 : 0;
		s.resize((size_t)first, 0x5a);
		for (int i = 0; i < n_rec; ++i) { starts.push_back(s.size()); record(s); }
		std::vector<uint64_t> hint(1, 0);
		for (size_t i = 1; i < starts.size(); ++i) if (rnd() % 4 == 0) hint.push_back(starts[i]);
		if (rnd() % 8 == 0) hint.push_back(hint.back());   /* an interval without bytes */
		const int kind = it < 300 ? -1 : (int)(rnd() % 6);
		const uint64_t at = starts[rnd() % starts.size()];
		if (kind == 0) { const uint32_t v = rnd() % 32; memcpy(s.data() + at, &v, 4); }
		else if (kind == 1) { const uint32_t v = rnd() & 1 ? 0xffffffffu : (uint32_t)(rnd() % (2 * s.size() + 64)); memcpy(s.data() + at, &v, 4); }
		else if (kind == 2) { s[(size_t)at + 12] = (uint8_t)rnd(); const uint16_t v = (uint16_t)rnd(); if (rnd() & 1) memcpy(s.data() + at + 16, &v, 2); }
		else if (kind == 3) { s.resize(s.size() - (1 + rnd() % std::min<size_t>(s.size() - (size_t)first - 1, 60))); }
		else if (kind == 4 && hint.size() > 1) { uint64_t &h = hint[1 + rnd() % (hint.size() - 1)]; h += 1 + rnd() % 30; std::sort(hint.begin(), hint.end()); }
		else if (kind == 5) { for (int j = 0; j < 3; ++j) s[(size_t)first + rnd() % (s.size() - (size_t)first)] ^= (uint8_t)(1u << (rnd() & 7)); }
		while (!hint.empty() && hint.back() > s.size()) hint.pop_back();
		if (hint.empty()) hint.push_back(0);
		hint.push_back(s.size());
		n_good += plain_walk(s, first).good;
		judge(s, hint, first, it);
	}
	if (n_fail) { fprintf(stderr, "bam_scan_fuzz: %ld checks failed\n", n_fail); return 1; }
	printf("bam_scan_fuzz: clean (3000 streams, %ld good by the plain walk)\n", n_good);
	return 0;
}
