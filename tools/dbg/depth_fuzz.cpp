/*
 * depth_fuzz.cpp -- memory safety and exactness of ssg_depth_* (k_depth.h) on the host emulation and under the sanitizers (never on a GPU: a stand-alone program,
 * `make fuzz-depth` builds and runs it).  3000 seeded cases: a stream of BAM-shaped records -- CIGARs of every operation code (unknown ones among them), tids
 * from -1 to 3, qualities of every byte, an l_seq of 0, shorter than the CIGAR's query and, on the quality path in every seventh case, one that leaves its record
 * -- in a chunk exactly as long as its records plus the store's 16 bytes of slack (a heap block of the emulation: the sanitizer sees a load behind it); one to
 * three spans over it, with every filter of a small set, quality floors 0, 1, 20 and 255 and LDS tiles of 0, 8 and 64 positions and the default.  A plain C++
 * restatement of the contract says what must come back: the numbers of a push, the counters, sums over random pairs with thresholds, and the text at its exact
 * length; a push into a chunk with a malformed record is SSG_EIO and leaves the counters as they were; every refusal of the arguments and of the state is asked
 * for once a case.  The sanitizers watch the rest.
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

static void record(bytes_t &s, int32_t tid, int32_t pos)
{
	const uint32_t l_qname = 1 + rnd() % 4, nc = rnd() % 12 == 0 ? 0 : 1 + rnd() % (rnd() % 8 == 0 ? 70 : 5);
	const uint32_t flag = (rnd() % 8 == 0 ? 0x4u : 0u) | (rnd() & 1 ? 0x10u : 0u) | (rnd() % 8 == 0 ? 0x100u : 0u) | (rnd() % 8 == 0 ? 0x200u : 0u) | (rnd() % 8 == 0 ? 0x400u : 0u);
	bytes_t body; uint32_t qlen = 0;
	for (uint32_t i = 0; i + 1 < l_qname; ++i) body.push_back('q');
	body.push_back(0);
	for (uint32_t i = 0; i < nc; ++i) {
		const uint32_t op = rnd() % 16 == 0 ? 9 + rnd() % 7 : rnd() % 3 == 0 ? rnd() % 9 : 0, len = rnd() % 10 == 0 ? 1 + rnd() % 400 : 1 + rnd() % 40, v = len << 4 | op;
		body.insert(body.end(), (const uint8_t*)&v, (const uint8_t*)&v + 4);
		if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) qlen += len;
	}
	const uint32_t l_seq = rnd() % 6 == 0 ? 0 : rnd() % 6 == 0 ? rnd() % (qlen + 1) : qlen;
	for (uint32_t i = 0; i < (l_seq + 1) / 2; ++i) body.push_back((uint8_t)rnd());
	const uint32_t qk = rnd() % 4;
	for (uint32_t i = 0; i < l_seq; ++i) body.push_back(qk == 0 ? 0xff : qk == 1 ? (uint8_t)rnd() : (uint8_t)(18 + rnd() % 5));
	for (uint32_t i = rnd() % 6; i > 0; --i) body.push_back((uint8_t)rnd());
	const uint32_t core[9] = { 32 + (uint32_t)body.size(), (uint32_t)tid, (uint32_t)pos, l_qname | (rnd() % 3 ? 30u : 0u) << 8, flag << 16 | nc, l_seq, 0xffffffffu, 0xffffffffu, 0 };
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
	F.push_back({ "the default", { fop(SSG_FOP_FLAG, 0, 0x704), fop(SSG_FOP_NOT, 0, 0) }, [](uint32_t f, uint32_t) { return !(f & 0x704); } });
	F.push_back({ "mapq and default", { fop(SSG_FOP_GE, SSG_FLD_MAPQ, 1), fop(SSG_FOP_FLAG, 0, 0x704), fop(SSG_FOP_NOT, 0, 0), fop(SSG_FOP_AND, 0, 0) }, [](uint32_t f, uint32_t q) { return q >= 1 && !(f & 0x704); } });
	F.push_back({ "reverse or duplicate", { fop(SSG_FOP_FLAG, 0, 0x10), fop(SSG_FOP_FLAG, 0, 0x400), fop(SSG_FOP_OR, 0, 0) }, [](uint32_t f, uint32_t) { return (f & 0x410) != 0; } });
	F.push_back({ "nothing", { fop(SSG_FOP_LT, SSG_FLD_SEQ_LEN, 0) }, [](uint32_t, uint32_t) { return false; } });
	return F;
}
struct plain_t { std::vector<uint32_t> span, cov; uint64_t n_rec, n_used, n_later, desc, behind; bool bad; };
static void plain_push(const bytes_t &s, const filter_t &F, int q, int32_t tid, int64_t beg, int64_t end, plain_t &P)
{
	P.n_rec = P.n_used = P.n_later = P.desc = P.behind = 0; P.bad = false;
	std::vector<uint32_t> sp = P.span, cv = P.cov;
	uint64_t prev = 0; bool first = true;
	for (uint64_t o = 0; o < s.size(); ) {
		uint32_t x[6]; memcpy(x, s.data() + o, 24);
		const uint64_t bs = x[0], lq = x[3] & 0xff, nc = x[4] & 0xffff, l = x[5];
		const int32_t t = (int32_t)x[1], pos = (int32_t)x[2]; const uint32_t flag = x[4] >> 16, mapq = x[3] >> 8 & 0xff;
		const uint8_t *cig = s.data() + o + 36 + lq, *qual = cig + 4 * nc + (l + 1) / 2;
		int64_t e = pos;
		for (uint64_t k = 0; k < nc; ++k) { uint32_t v; memcpy(&v, cig + 4 * k, 4); const uint32_t op = v & 15; if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) e += v >> 4; }
		if ((flag & 4) || nc == 0) e = (int64_t)pos + 1;   /* bam_endpos, as the scan's entry has it */
		const uint64_t key = ((uint64_t)(uint32_t)t << 32 | ((uint64_t)(uint32_t)(pos + 1) << 1 & 0xffffffffu)) >> 1;
		if (!first && key < prev) ++P.desc;
		prev = key; first = false; ++P.n_rec;
		if (t < 0 || t > tid || (t == tid && pos >= end)) ++P.behind;
		const bool pass = F.keeps(flag, mapq) && t >= 0 && nc > 0;
		if (pass && (t > tid || (t == tid && e > end))) ++P.n_later;
		if (pass && t == tid && pos < end && e > beg) {
			++P.n_used;
			if (q > 0 && 32 + lq + 4 * nc + (l + 1) / 2 + l > bs) P.bad = true;
			int64_t r = pos, qi = 0;
			for (uint64_t k = 0; k < nc && !P.bad; ++k) {
				uint32_t v; memcpy(&v, cig + 4 * k, 4); const uint32_t op = v & 15; const int64_t len = v >> 4;
				const bool ro = op == 0 || op == 2 || op == 3 || op == 7 || op == 8, bo = op == 0 || op == 7 || op == 8;
				if (ro) for (int64_t i = std::max<int64_t>(0, beg - r); i < len && r + i < end; ++i) {
					++sp[(size_t)(r + i - beg)];
					if (bo && (q == 0 || qi + i >= (int64_t)l || qual[qi + i] >= q)) ++cv[(size_t)(r + i - beg)];
				}
				if (ro) r += len;
				if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) qi += len;
			}
		}
		o += 4 + bs;
	}
	if (!P.bad) { P.span.swap(sp); P.cov.swap(cv); }
}

static void refusals(ssg_recs_t *r, ssg_depth_t *d, uint32_t cid, const uint64_t *hint, int64_t n_hints)
{	/* d has no span */
	ssg_depth_t *x = 0; uint64_t a, b, c, e, len; uint32_t u; uint8_t byte;
	const ssg_bam_fop_t under[1] = { fop(SSG_FOP_AND, 0, 0) }, two[2] = { fop(SSG_FOP_FLAG, 0, 1), fop(SSG_FOP_FLAG, 0, 2) }, unk[1] = { fop(12, 0, 0) }, fld[1] = { fop(SSG_FOP_EQ, 9, 0) };
	EXPECT(ssg_depth_create(r, under, 1, 0, &x) == SSG_EINVAL && ssg_depth_create(r, two, 2, 0, &x) == SSG_EINVAL && ssg_depth_create(r, unk, 1, 0, &x) == SSG_EINVAL && ssg_depth_create(r, fld, 1, 0, &x) == SSG_EINVAL, "a bad program was taken");
	EXPECT(ssg_depth_create(r, 0, 0, -1, &x) == SSG_EINVAL && ssg_depth_create(r, 0, 0, 256, &x) == SSG_EINVAL && ssg_depth_create(0, 0, 0, 0, &x) == SSG_EINVAL, "a bad min_baseq or store was taken");
	EXPECT(ssg_depth_push(d, cid, hint, n_hints, 0, &a, &b, &c, &e, 0) == SSG_EINVAL && ssg_depth_finish(d) == SSG_EINVAL && ssg_depth_end(d) == SSG_EINVAL, "a call without a span was taken");
	EXPECT(ssg_depth_get(d, 0, 1, &u, &u) == SSG_EINVAL && ssg_depth_sums(d, 0, 0, 0, 0, 0) == SSG_EINVAL && ssg_depth_text(d, "x", 0, 1, 0, &byte, 1, &len) == SSG_EINVAL, "a result without a span was given");
	EXPECT(ssg_depth_begin(d, -1, 0, 5) == SSG_EINVAL && ssg_depth_begin(d, 0, -1, 5) == SSG_EINVAL && ssg_depth_begin(d, 0, 5, 5) == SSG_EINVAL && ssg_depth_begin(d, 0, 0, (int64_t)1 << 31) == SSG_EINVAL, "a bad span was opened");
	EXPECT(ssg_depth_begin(d, 0, 3, 9) == 0 && ssg_depth_begin(d, 0, 3, 9) == SSG_EINVAL, "two spans at once");
	EXPECT(ssg_depth_push(d, cid + 7, hint, n_hints, 0, &a, &b, &c, &e, 0) == SSG_EINVAL, "a chunk that does not exist was pushed");
	EXPECT(ssg_depth_get(d, 3, 9, &u, &u) == SSG_EINVAL, "counters before finish");
	EXPECT(ssg_depth_finish(d) == 0 && ssg_depth_finish(d) == SSG_EINVAL && ssg_depth_push(d, cid, hint, n_hints, 0, &a, &b, &c, &e, 0) == SSG_EINVAL, "finish twice, or a push behind it");
	const int64_t out1[2] = { 2, 5 }, out2[2] = { 5, 10 }, empty[2] = { 5, 5 }; uint64_t o3[3];
	EXPECT(ssg_depth_sums(d, out1, 1, 0, 0, o3) == SSG_EINVAL && ssg_depth_sums(d, out2, 1, 0, 0, o3) == SSG_EINVAL && ssg_depth_sums(d, empty, 1, 0, 0, o3) == SSG_EINVAL && ssg_depth_sums(d, out1, 1, &u, 9, o3) == SSG_EINVAL, "a bad pair or threshold count was taken");
	EXPECT(ssg_depth_get(d, 2, 9, &u, &u) == SSG_EINVAL && ssg_depth_get(d, 3, 10, &u, &u) == SSG_EINVAL && ssg_depth_text(d, "x", 2, 9, 1, 0, 0, &len) == SSG_EINVAL && ssg_depth_text(d, "", 3, 9, 1, 0, 0, &len) == SSG_EINVAL, "positions outside the span were taken");
	EXPECT(ssg_depth_end(d) == 0, "end");
}

int main()
{
	const std::vector<filter_t> F = filters();
	long n_spans = 0, n_eio = 0; uint64_t n_used_all = 0, n_text_all = 0;
	for (int c = 0; c < 3000; ++c) {
		rng_s = 0x9e3779b97f4a7c15ull ^ ((uint64_t)(c + 1) * 0x2545f4914f6cdd1dull);
		const filter_t &flt = F[rnd() % F.size()];
		static const int QS[] = { 0, 0, 1, 20, 255 }; const int q = QS[rnd() % 5];
		static const char *const TILES[] = { "0", "8", "64", 0 }; const char *const tile = TILES[rnd() % 4];
		if (tile) setenv("SSG_DEPTH_TILE", tile, 1); else unsetenv("SSG_DEPTH_TILE");
		/* the stream: sorted or not, dense or sparse */
		bytes_t s; std::vector<uint64_t> starts;
		const uint32_t n = rnd() % 400, spread = rnd() % 3 == 0 ? 5000 : 300; const bool sorted = rnd() % 4 != 0;
		std::vector<std::pair<int32_t, int32_t> > at;
		for (uint32_t i = 0; i < n; ++i) at.push_back(std::make_pair((int32_t)(rnd() % 16 == 0 ? 3 : rnd() % 3), (int32_t)(rnd() % spread)));
		if (sorted) std::sort(at.begin(), at.end());
		for (uint32_t i = 0; i < n; ++i) { starts.push_back(s.size()); record(s, at[i].first, at[i].second); }
		for (uint32_t i = rnd() % 4; i > 0 && sorted; --i) { starts.push_back(s.size()); record(s, -1, -1); }
		bool broken = false;
		if (!starts.empty() && c % 7 == 0) {   /* a sequence that leaves its record */
			const uint64_t o = starts[rnd() % starts.size()]; uint32_t x[6]; memcpy(x, s.data() + o, 24);
			const uint64_t room = x[0] - 32 - (x[3] & 0xff) - 4 * (uint64_t)(x[4] & 0xffff);
			uint32_t l = 0; while (((uint64_t)l + 1) / 2 + l <= room) ++l;
			if (rnd() % 3 == 0) l = 0x7fffffffu; else l += rnd() % 50;
			memcpy(s.data() + o + 20, &l, 4); broken = true;
		}
		std::vector<uint64_t> hint;
		for (size_t i = 0; i < starts.size(); ++i) if (i == 0 || rnd() % 3 == 0) hint.push_back(starts[i]);
		if (hint.empty()) hint.push_back(0);
		hint.push_back(s.size());
		ssg_recs_t *r = 0; ssg_depth_t *d = 0; uint32_t cid = 0;
		if (ssg_recs_create(~(uint64_t)0 >> 1, &r) || ssg_depth_create(r, flt.prog.empty() ? 0 : flt.prog.data(), (int)flt.prog.size(), q, &d) || ssg_recs_append(r, s.data(), s.size(), &cid)) { EXPECT(0, "create: %s", ssg_err_msg.c_str()); return 1; }
		refusals(r, d, cid, hint.data(), (int64_t)hint.size() - 1);
		for (uint32_t k = 1 + rnd() % 3; k > 0; --k) {
			const int32_t tid = (int32_t)(rnd() % 4); const int64_t beg = rnd() % 4 == 0 ? 0 : rnd() % spread, end = beg + 1 + (rnd() % 5 == 0 ? 0 : rnd() % (2 * spread));
			const int64_t np = end - beg;
			plain_t P; P.span.assign((size_t)np, 0); P.cov.assign((size_t)np, 0);
			EXPECT(ssg_depth_begin(d, tid, beg, end) == 0, "case %d: begin: %s", c, ssg_err_msg.c_str());
			const uint32_t pushes = 1 + rnd() % 2;
			bool eio = false;
			for (uint32_t p = 0; p < pushes; ++p) {
				uint64_t n_rec = 0, n_used = 0, n_later = 0, desc = 0, behind = 0;
				plain_push(s, flt, q, tid, beg, end, P);
				const int rc = ssg_depth_push(d, cid, hint.data(), (int64_t)hint.size() - 1, 0, &n_rec, &n_used, &n_later, &desc, &behind);
				if (P.bad) { eio = true; EXPECT(rc == SSG_EIO && broken && ssg_err_msg.find("l_seq") != std::string::npos, "case %d: rc %d (%s), a malformed record is used", c, rc, ssg_err_msg.c_str()); continue; }
				EXPECT(rc == 0, "case %d: push: rc %d (%s)", c, rc, ssg_err_msg.c_str());
				EXPECT(n_rec == P.n_rec && n_used == P.n_used && n_later == P.n_later && desc == P.desc && behind == P.behind, "case %d: push gave %llu %llu %llu %llu %llu, wanted %llu %llu %llu %llu %llu", c,
				       (unsigned long long)n_rec, (unsigned long long)n_used, (unsigned long long)n_later, (unsigned long long)desc, (unsigned long long)behind,
				       (unsigned long long)P.n_rec, (unsigned long long)P.n_used, (unsigned long long)P.n_later, (unsigned long long)P.desc, (unsigned long long)P.behind);
				n_used_all += n_used;
			}
			n_eio += eio; ++n_spans;
			EXPECT(ssg_depth_finish(d) == 0, "case %d: finish: %s", c, ssg_err_msg.c_str());
			std::vector<uint32_t> gs((size_t)np), gc((size_t)np);   /* exactly as long as asked: a store behind them is the sanitizer's */
			EXPECT(ssg_depth_get(d, beg, end, gs.data(), gc.data()) == 0 && gs == P.span && gc == P.cov, "case %d (%s, q %d, tile %s): the counters of %d:%lld-%lld differ", c, flt.what, q, tile ? tile : "default", tid, (long long)beg, (long long)end);
			/* sums */
			std::vector<int64_t> reg; std::vector<uint32_t> thr; std::vector<uint64_t> want;
			const uint32_t n_reg = rnd() % 6, n_thr = rnd() % 9;
			for (uint32_t t = 0; t < n_thr; ++t) thr.push_back(rnd() % 4 == 0 ? 0 : rnd() % 12);
			for (uint32_t g = 0; g < n_reg; ++g) {
				const int64_t b = beg + rnd() % np, e = b + 1 + rnd() % (end - b);
				reg.push_back(b); reg.push_back(e);
				uint64_t ss = 0, sc = 0; std::vector<uint64_t> cn(n_thr, 0);
				for (int64_t p = b; p < e; ++p) { ss += P.span[(size_t)(p - beg)]; sc += P.cov[(size_t)(p - beg)]; for (uint32_t t = 0; t < n_thr; ++t) cn[t] += P.cov[(size_t)(p - beg)] >= thr[t]; }
				want.push_back(ss); want.push_back(sc); want.insert(want.end(), cn.begin(), cn.end());
			}
			std::vector<uint64_t> got(want.size());
			EXPECT(ssg_depth_sums(d, reg.data(), n_reg, thr.data(), (int)n_thr, got.data()) == 0 && got == want, "case %d: the sums differ (%s)", c, ssg_err_msg.c_str());
			/* text */
			const int64_t p0 = beg + rnd() % np, p1 = p0 + rnd() % (end - p0 + 1); const int all = rnd() & 1;
			const std::string name = rnd() % 5 == 0 ? std::string(255, 'n') : "ctg";
			std::string wt;
			for (int64_t p = p0; p < p1; ++p) if (all || P.span[(size_t)(p - beg)]) wt += name + "\t" + std::to_string(p + 1) + "\t" + std::to_string(P.cov[(size_t)(p - beg)]) + "\n";
			uint64_t len = 0;
			EXPECT(ssg_depth_text(d, name.c_str(), p0, p1, all, 0, 0, &len) == 0 && len == wt.size(), "case %d: the sizing form gave %llu, wanted %zu", c, (unsigned long long)len, wt.size());
			bytes_t out(wt.size());
			EXPECT(ssg_depth_text(d, name.c_str(), p0, p1, all, out.data(), out.size(), &len) == 0 && len == wt.size() && (wt.empty() || !memcmp(out.data(), wt.data(), wt.size())), "case %d: the text differs (%s)", c, ssg_err_msg.c_str());
			if (!wt.empty()) EXPECT(ssg_depth_text(d, name.c_str(), p0, p1, all, out.data(), out.size() - 1, &len) == SSG_EOVERFLOW && len == wt.size(), "case %d: a buffer one byte short was taken", c);
			n_text_all += wt.size();
			EXPECT(ssg_depth_end(d) == 0, "case %d: end", c);
		}
		ssg_depth_free(d);
		ssg_recs_free(r);
	}
	printf("depth_fuzz: 3000 cases: %ld spans, %llu records added, %llu bytes of text, %ld spans met SSG_EIO; %ld failures\n", n_spans, (unsigned long long)n_used_all, (unsigned long long)n_text_all, n_eio, n_fail);
	return n_fail ? 1 : 0;
}
