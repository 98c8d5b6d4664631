/*
 * bam_select_fuzz.cpp -- memory safety and exactness of ssg_recs_select (k_bam_select.h) on the host emulation and under the sanitizers (never on a GPU: a
 * stand-alone program, `make fuzz-bam-select` builds and runs it).  3000 seeded cases: a stream of BAM-shaped records in a chunk that is exactly as long as the
 * stream plus the store's 16 bytes of slack (a heap block of the emulation: the sanitizer sees a load behind it), hints at record starts, a random list of
 * sorted, disjoint regions (or none) and a random valid postfix program (or none); every seventh case carries one of the refusals instead -- regions that are
 * unsorted, overlap, touch, are empty or have no contig, a program that is too long, underflows, leaves two values, or names an unknown operation or field.
 * A plain loop over the stream decides what is kept: the return code, both counts and loc / key / ent of every kept record must match it exactly, the counting
 * form must give the same counts, and one record less of room must be SSG_EOVERFLOW with nothing written.  The sanitizers watch the rest.
 * Second part, the .bai reader (bai_reader_t, host/bamio.h) on a real index -- the one bai_t makes of 6000 sorted records over three contigs: parsed whole, the
 * candidate chunks of 2000 random regions must hold the virtual offset of every record that overlaps the region; every seeded truncation must be refused
 * (all but the one that only drops the optional count of unplaced reads, which is a complete index); 3000 seeded mutations -- bytes flipped, counts made huge
 * or negative -- are refused or parsed, and a parsed one is queried: no outcome may be a crash or a read outside the file's bytes.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/ssgpu.h"
#include "../../speedseq_amd/host/bamio.h"
#include <unistd.h>

thread_local std::string ssg_err_msg;      /* what ssgpu_core.cpp defines for the library */
thread_local int ssg_cur_dev = 0;
thread_local int ssg_lane = 0;

typedef std::vector<uint8_t> bytes_t;
static uint64_t rng_s = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rng_s ^= rng_s << 13; rng_s ^= rng_s >> 7; rng_s ^= rng_s << 17; return (uint32_t)(rng_s >> 16); }
static long n_fail = 0;
#define EXPECT(c, ...) do { if (!(c)) { if (++n_fail < 20) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static const int32_t MAPQS[] = { 0, 1, 19, 20, 21, 60, 254, 255 }, TLENS[] = { -501, -500, -1, 0, 1, 499, 500 };

static void record(bytes_t &s)
{
	const uint32_t l_qname = 1 + rnd() % 12, nc = rnd() % 6, l_seq = rnd() % 40, flag = (rnd() % 3 == 0 ? rnd() & 0xfffu : 0u) | (rnd() & 1 ? 16u : 0u) | (rnd() % 7 == 0 ? 4u : 0u);
	const uint32_t bs = 32 + l_qname + 4 * nc + (l_seq + 1) / 2 + l_seq + rnd() % 9;
	uint32_t core[9] = { bs, (uint32_t)((int32_t)(rnd() % 4) - 1), rnd() % 8 == 0 ? 0xffffffffu : rnd() % 3000u, l_qname | (uint32_t)MAPQS[rnd() % 8] << 8 | (rnd() & 0xffffu) << 16, flag << 16 | nc, l_seq,
	                     (uint32_t)((int32_t)(rnd() % 4) - 1), rnd() % 3000u, (uint32_t)TLENS[rnd() % 7] };
	s.insert(s.end(), (uint8_t*)core, (uint8_t*)core + 36);
	for (uint32_t i = 0; i < l_qname; ++i) s.push_back(i + 1 < l_qname ? 'q' : 0);
	for (uint32_t i = 0; i < nc; ++i) { const uint32_t v = (rnd() % 90) << 4 | rnd() % 9; s.insert(s.end(), (uint8_t*)&v, (uint8_t*)&v + 4); }
	const size_t rest = bs - 32 - l_qname - 4 * nc;
	for (size_t i = 0; i < rest; ++i) s.push_back((uint8_t)rnd());
}

struct one_t { uint64_t off, key; ssg_bam_ent_t ent; int32_t mapq, l_seq, mtid, isize; };
/* the plain walk of a good stream */
static std::vector<one_t> plain_walk(const bytes_t &s, uint64_t first)
{
	std::vector<one_t> w; uint64_t o = first;
	while (o < s.size()) {
		uint32_t x[9]; memcpy(x, s.data() + o, 36);
		const uint32_t l_qname = x[3] & 0xff, nc = x[4] & 0xffff, flag = x[4] >> 16;
		int32_t end = (int32_t)x[2] + 1;
		if (!(flag & 4) && nc) { int32_t rl = 0; for (uint32_t i = 0; i < nc; ++i) { uint32_t v; memcpy(&v, s.data() + o + 36 + l_qname + 4 * i, 4); const uint32_t op = v & 15; if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += (int32_t)(v >> 4); } end = (int32_t)x[2] + rl; }
		one_t r; r.off = o; r.ent.tid = (int32_t)x[1]; r.ent.pos = (int32_t)x[2]; r.ent.end = end; r.ent.flag = flag; r.ent.len = 4 + x[0]; r.ent.pad = 0;
		r.key = (uint64_t)(int64_t)(int32_t)x[1] << 32 | (uint64_t)(uint32_t)((x[2] + 1u) << 1) | (flag & 16 ? 1u : 0u);
		r.mapq = (int32_t)(x[3] >> 8 & 0xff); r.l_seq = (int32_t)x[5]; r.mtid = (int32_t)x[6]; r.isize = (int32_t)x[8];
		w.push_back(r);
		o += 4 + (uint64_t)x[0];
	}
	return w;
}

/* the decision in plain C++: every region tried, the program on a vector of booleans */
static bool plain_keep(const one_t &r, const std::vector<ssg_bam_region_t> &reg, const std::vector<ssg_bam_fop_t> &prog)
{
	if (!reg.empty()) {
		bool in = false;
		for (size_t k = 0; k < reg.size(); ++k) if (r.ent.tid >= 0 && reg[k].tid == r.ent.tid && r.ent.pos < reg[k].end && r.ent.end > reg[k].beg) in = true;
		if (!in) return false;
	}
	if (prog.empty()) return true;
	std::vector<bool> st;
	for (size_t pc = 0; pc < prog.size(); ++pc) {
		const ssg_bam_fop_t &f = prog[pc];
		if (f.op == SSG_FOP_FLAG) st.push_back(((int32_t)r.ent.flag & f.value) != 0);
		else if (f.op == SSG_FOP_NOT) st.back() = !st.back();
		else if (f.op == SSG_FOP_AND || f.op == SSG_FOP_OR) { const bool b = st.back(); st.pop_back(); st.back() = f.op == SSG_FOP_AND ? (st.back() && b) : (st.back() || b); }
		else {
			const int32_t v = f.arg == SSG_FLD_MAPQ ? r.mapq : f.arg == SSG_FLD_REF_ID ? r.ent.tid : f.arg == SSG_FLD_MATE_REF_ID ? r.mtid : f.arg == SSG_FLD_TLEN ? r.isize : f.arg == SSG_FLD_SEQ_LEN ? r.l_seq : (int32_t)r.ent.flag;
			st.push_back(f.op == SSG_FOP_EQ ? v == f.value : f.op == SSG_FOP_NE ? v != f.value : f.op == SSG_FOP_LT ? v < f.value : f.op == SSG_FOP_LE ? v <= f.value : f.op == SSG_FOP_GT ? v > f.value : v >= f.value);
		}
	}
	return st.back();
}

static ssg_bam_fop_t fop(int op, int arg, int32_t value) { ssg_bam_fop_t f; f.op = (uint8_t)op; f.arg = (uint8_t)arg; f.pad = 0; f.value = value; return f; }
static ssg_bam_fop_t random_push()
{
	if (rnd() % 3 == 0) return fop(SSG_FOP_FLAG, 0, rnd() % 4 == 0 ? (int32_t)(rnd() & 0xfff) : 1 << rnd() % 12);
	const int arg = (int)(rnd() % 6);
	const int32_t v = arg == SSG_FLD_MAPQ ? MAPQS[rnd() % 8] + (int32_t)(rnd() % 3) - 1 : arg == SSG_FLD_TLEN ? TLENS[rnd() % 7] + (int32_t)(rnd() % 3) - 1 : arg == SSG_FLD_SEQ_LEN ? (int32_t)(rnd() % 41)
	                : arg == SSG_FLD_FLAG ? (int32_t)(rnd() & 0x1f) : (int32_t)(rnd() % 5) - 2;
	return fop(SSG_FOP_EQ + (int)(rnd() % 6), arg, v);
}
/* a valid program of exactly `len' operations: the depth never exceeds what the operations left can bring back to one */
static std::vector<ssg_bam_fop_t> random_program(int len)
{
	std::vector<ssg_bam_fop_t> p; int depth = 0;
	for (int left = len; left > 0; --left) {
		const bool may_push = depth <= left - 1, may_not = depth >= 1 && depth - 1 <= left - 1, may_bin = depth >= 2;
		for (;;) {
			const uint32_t c = rnd() % 8;
			if (c < 4 && may_push) { p.push_back(random_push()); ++depth; break; }
			if (c == 4 && may_not) { p.push_back(fop(SSG_FOP_NOT, 0, 0)); break; }
			if (c > 4 && may_bin) { p.push_back(fop(rnd() & 1 ? SSG_FOP_AND : SSG_FOP_OR, 0, 0)); --depth; break; }
		}
	}
	return p;
}
static std::vector<ssg_bam_region_t> random_regions(int n)
{
	std::vector<ssg_bam_region_t> g; int32_t tid = 0, at = (int32_t)(rnd() % 200);
	for (int k = 0; k < n; ++k) {
		if (rnd() % 5 == 0) { tid += 1 + (int32_t)(rnd() % 2); at = (int32_t)(rnd() % 200); }
		ssg_bam_region_t r; r.tid = tid; r.beg = at; r.end = at + 1 + (int32_t)(rnd() % 150);
		g.push_back(r); at = r.end + 1 + (int32_t)(rnd() % 120);
	}
	return g;
}

struct got_t { int rc; uint64_t n_rec, n_sel; std::vector<uint64_t> loc, key; std::vector<ssg_bam_ent_t> ent; };
static got_t run(ssg_recs_t *r, uint32_t cid, const std::vector<uint64_t> &hint, uint64_t first, const std::vector<ssg_bam_region_t> &reg, const std::vector<ssg_bam_fop_t> &prog, size_t cap, bool counting)
{
	got_t g; g.n_rec = g.n_sel = 77;
	/* exactly cap elements: a store behind them is the sanitizer's to see */
	g.loc.assign(cap, 0xabababababababab); g.key.assign(cap, 0xabababababababab); ssg_bam_ent_t z; memset(&z, 0xab, sizeof(z)); g.ent.assign(cap, z);
	void *const none = malloc(1);   /* arrays without room (cap == 0 with arrays is not the counting form): a block of one byte */
	g.rc = ssg_recs_select(r, cid, hint.data(), (int64_t)hint.size() - 1, first, reg.empty() ? 0 : reg.data(), (int64_t)reg.size(), prog.empty() ? 0 : prog.data(), (int)prog.size(),
	                       counting ? 0 : cap, &g.n_rec, &g.n_sel, counting ? 0 : cap ? g.loc.data() : (uint64_t*)none, counting ? 0 : cap ? g.key.data() : (uint64_t*)none, counting ? 0 : cap ? g.ent.data() : (ssg_bam_ent_t*)none);
	free(none);
	return g;
}
static bool untouched(const got_t &g)
{
	for (size_t i = 0; i < g.loc.size(); ++i) if (g.loc[i] != 0xabababababababab || g.key[i] != 0xabababababababab || g.ent[i].pad != 0xabababab) return false;
	return true;
}

/* ---- the .bai reader ---- */
struct placed_t { int tid, beg, end; uint64_t v; };
static int bai_part()
{
	/* a real index: sorted records, every one 40 to 1200 bases long, virtual offsets that grow as a file's do */
	std::vector<placed_t> recs; const int n_ref = 4;   /* (the last contig has no record) */
	uint64_t v = (uint64_t)300 << 16 | 120;
	bai_t idx(n_ref, v);
	bool have = false; placed_t p = { 0, 0, 0, 0 };
	for (int tid = 0; tid < 3; ++tid) {
		int pos = (int)(rnd() % 5000);
		for (int i = 0; i < 2000; ++i) {
			placed_t r = { tid, pos, pos + 40 + (int)(rnd() % (rnd() % 9 == 0 ? 1160 : 100)), v };
			if (have && idx.push(p.tid, p.beg, p.end, v, true) < 0) { fprintf(stderr, "bam_select_fuzz: bai_t refused sorted records\n"); return 1; }
			p = r; have = true; recs.push_back(r);
			pos += (int)(rnd() % (rnd() % 50 == 0 ? 60000 : 300));
			const uint64_t in = (v & 0xffff) + 150 + rnd() % 200;            /* the next record's place: the same block, or the next */
			v = in >= 0xff00 ? ((v >> 16) + 9000 + rnd() % 9000) << 16 : (v & ~(uint64_t)0xffff) | in;
		}
	}
	idx.push(p.tid, p.beg, p.end, v, true); idx.finish(v);
	char path[] = "/tmp/bam_select_fuzz_XXXXXX";
	const int fd = mkstemp(path);
	if (fd < 0) { perror("mkstemp"); return 1; }
	close(fd); idx.save(path);
	std::vector<uint8_t> full; { FILE *f = fopen(path, "rb"); uint8_t b[65536]; size_t k; while ((k = fread(b, 1, sizeof(b), f)) > 0) full.insert(full.end(), b, b + k); fclose(f); }
	unlink(path);
	bai_reader_t R; std::string err;
	/* the sanitizer sees a read behind the bytes: each case is a heap block of exactly its length */
	auto parse = [&](const std::vector<uint8_t> &b) { uint8_t *h = (uint8_t*)malloc(b.size() ? b.size() : 1); if (b.size()) memcpy(h, b.data(), b.size()); const bool ok = R.parse(h, b.size(), err); free(h); return ok; };
	EXPECT(parse(full) && (int)R.refs.size() == n_ref, "the whole index (%zu bytes) is refused: %s", full.size(), err.c_str());
	long n_chunks = 0;
	for (int it = 0; it < 2000; ++it) {
		const int tid = (int)(rnd() % n_ref); const int64_t beg = rnd() % 700000, end = beg + 1 + (rnd() % 3 == 0 ? rnd() % 200000 : rnd() % 3000);
		std::vector<bai_reader_t::chunk_t> c; R.query(tid, beg, end, c); bai_chunks_merge(c); n_chunks += (long)c.size();
		for (size_t k = 1; k < c.size(); ++k) EXPECT(c[k - 1].v < c[k].u, "%d: merged chunks that are not apart", it);
		for (const placed_t &r : recs) if (r.tid == tid && r.beg < end && r.end > beg) {
			bool in = false;
			for (const bai_reader_t::chunk_t &x : c) if (x.u <= r.v && r.v < x.v) in = true;
			EXPECT(in, "%d: the record at %d:%d-%d (offset %llx) is in no chunk of %d:%lld-%lld", it, r.tid, r.beg, r.end, (unsigned long long)r.v, tid, (long long)beg, (long long)end);
		}
	}
	long n_trunc = 0, n_parsed = 0;
	for (int it = 0; it < 1500; ++it) {
		const size_t len = it < 64 ? (size_t)it : it < 128 ? full.size() - 1 - (size_t)(it - 64) : rnd() % full.size();
		if (len == full.size() - 8) continue;                              /* (the index without its optional last count) */
		std::vector<uint8_t> b(full.begin(), full.begin() + (ptrdiff_t)len);
		EXPECT(!parse(b), "a truncation to %zu of %zu bytes is taken", len, full.size()); ++n_trunc;
	}
	for (int it = 0; it < 3000; ++it) {
		std::vector<uint8_t> b = full;
		const int kind = (int)(rnd() % 4);
		if (kind == 0) for (int j = 0; j < 1 + (int)(rnd() % 4); ++j) b[rnd() % b.size()] ^= (uint8_t)(1u << (rnd() & 7));
		else if (kind == 1) { const int32_t big = rnd() & 1 ? 0x7fffffff : (int32_t)(rnd() % 3 == 0 ? -1 : 1 << (10 + rnd() % 20)); memcpy(b.data() + 4 * (rnd() % (b.size() / 4)), &big, 4); }
		else if (kind == 2) { const int32_t big = (int32_t)(rnd() % 2 ? 0x7fffffff : 0x10000000); memcpy(b.data() + 4 * (1 + rnd() % 4), &big, 4); }   /* n_ref, the first n_bin, bin, n_chunk */
		else { const size_t at = rnd() % b.size(), n = 1 + rnd() % 64; for (size_t j = at; j < at + n && j < b.size(); ++j) b[j] = (uint8_t)rnd(); }
		if (!parse(b)) continue;
		++n_parsed;
		for (int q = 0; q < 8; ++q) { std::vector<bai_reader_t::chunk_t> c; const int64_t beg = rnd() % 800000; R.query((int)(rnd() % (R.refs.size() + 1)) - (q == 0), beg, beg + 1 + rnd() % 100000, c); bai_chunks_merge(c); n_chunks += (long)c.size(); }
	}
	if (n_fail) return 1;
	printf("bam_select_fuzz: the .bai reader is clean (%zu bytes; 2000 regions, %ld chunks; %ld truncations refused; 3000 mutations, %ld parsed)\n", full.size(), n_chunks, n_trunc, n_parsed);
	return 0;
}

int main()
{
	long n_kept = 0, n_seen = 0, n_refused = 0;
	for (int it = 0; it < 3000; ++it) {
		bytes_t s; std::vector<uint64_t> starts;
		const int n_rec = it % 50 == 0 ? 250 + (int)(rnd() % 600) : 1 + (int)(rnd() % 90);
		const uint64_t first = rnd() % 3 == 0 ? 1 + rnd() % 50 : 0;
		s.resize((size_t)first, 0x5a);
		for (int i = 0; i < n_rec; ++i) { starts.push_back(s.size()); record(s); }
		std::vector<uint64_t> hint(1, 0);
		for (size_t i = 1; i < starts.size(); ++i) if (rnd() % 4 == 0) hint.push_back(starts[i]);
		if (rnd() % 8 == 0) hint.push_back(hint.back());   /* an interval without bytes */
		hint.push_back(s.size());
		std::vector<ssg_bam_region_t> reg = random_regions(rnd() % 4 == 0 ? 0 : rnd() % 8 == 0 ? 65 + (int)(rnd() % 200) : 1 + (int)(rnd() % 12));
		std::vector<ssg_bam_fop_t> prog = random_program(rnd() % 5 == 0 ? 0 : rnd() % 6 == 0 ? 64 : 1 + (int)(rnd() % 64));
		ssg_recs_t *r = 0; uint32_t cid = 0;
		if (ssg_recs_create(s.size(), &r) || ssg_recs_append(r, s.data(), s.size(), &cid)) { EXPECT(0, "store: %s", ssg_err_msg.c_str()); return 1; }
		const std::vector<one_t> w = plain_walk(s, first);
		if (it % 7 == 3) {   /* a refusal: one thing wrong, everything else as it was */
			const int kind = (it / 7) % 12;
			if (reg.size() < 2) reg = random_regions(3);
			const size_t k = 1 + rnd() % (reg.size() - 1);
			if (kind == 0) std::swap(reg[k - 1], reg[k]);
			else if (kind == 1) { reg[k].tid = reg[k - 1].tid; reg[k].beg = reg[k - 1].end - 1; if (reg[k].end <= reg[k].beg) reg[k].end = reg[k].beg + 1; }
			else if (kind == 2) { reg[k].tid = reg[k - 1].tid; reg[k].beg = reg[k - 1].end; if (reg[k].end <= reg[k].beg) reg[k].end = reg[k].beg + 1; }
			else if (kind == 3) reg[k].end = reg[k].beg - (int32_t)(rnd() % 2);
			else if (kind == 4) reg[0].tid = -1;
			else if (kind == 5) { prog = random_program(64); prog.insert(prog.begin() + 1, fop(SSG_FOP_NOT, 0, 0)); }
			else if (kind == 6) { prog = random_program(1 + (int)(rnd() % 30)); prog.insert(prog.begin() + (rnd() & 1), fop(SSG_FOP_AND + (int)(rnd() % 3), 0, 0)); if (prog[0].op == SSG_FOP_FLAG || prog[0].op >= SSG_FOP_EQ) prog.insert(prog.begin(), fop(SSG_FOP_OR, 0, 0)); }
			else if (kind == 7) { prog = random_program(1 + (int)(rnd() % 30)); prog.push_back(random_push()); }
			else if (kind == 8) { prog = random_program(1 + (int)(rnd() % 30)); prog[rnd() % prog.size()].op = (uint8_t)(10 + rnd() % 246); }
			else if (kind == 9) { prog = random_program(1 + (int)(rnd() % 30)); size_t j = 0; while (prog[j].op < SSG_FOP_EQ && j + 1 < prog.size()) ++j; prog[j] = fop(SSG_FOP_EQ + (int)(rnd() % 6), 6 + (int)(rnd() % 250), 0); }
			else if (kind == 10) { prog.clear(); prog.push_back(random_push()); prog.push_back(random_push()); prog.push_back(random_push()); prog.push_back(fop(SSG_FOP_AND, 0, 0)); }
			else { prog.clear(); prog.push_back(random_push()); prog.push_back(fop(SSG_FOP_OR, 0, 0)); prog.push_back(random_push()); }
			const got_t g = run(r, cid, hint, first, reg, prog, w.size(), false);
			EXPECT(g.rc == SSG_EINVAL && g.n_rec == 0 && g.n_sel == 0 && untouched(g), "%d: refusal %d: rc %d (%s), %llu scanned, %llu kept", it, kind, g.rc, ssg_err_msg.c_str(), (unsigned long long)g.n_rec, (unsigned long long)g.n_sel);
			const got_t c = run(r, cid, hint, first, reg, prog, 0, true);
			EXPECT(c.rc == SSG_EINVAL, "%d: refusal %d, counting: rc %d", it, kind, c.rc);
			++n_refused;
			ssg_recs_free(r);
			continue;
		}
		std::vector<size_t> keep;
		for (size_t i = 0; i < w.size(); ++i) if (plain_keep(w[i], reg, prog)) keep.push_back(i);
		n_seen += (long)w.size(); n_kept += (long)keep.size();
		const got_t g = run(r, cid, hint, first, reg, prog, keep.size(), false);   /* exactly the room that is needed */
		EXPECT(g.rc == 0 && g.n_rec == w.size() && g.n_sel == keep.size(), "%d: rc %d (%s), %llu of %llu, expected %zu of %zu", it, g.rc, ssg_err_msg.c_str(), (unsigned long long)g.n_sel, (unsigned long long)g.n_rec, keep.size(), w.size());
		if (g.rc == 0 && g.n_sel == keep.size())
			for (size_t j = 0; j < keep.size(); ++j) {
				const one_t &o = w[keep[j]];
				EXPECT(g.loc[j] == ((uint64_t)cid << 40 | o.off) && g.key[j] == o.key && !memcmp(&g.ent[j], &o.ent, sizeof(o.ent)), "%d: kept record %zu differs", it, j);
			}
		const got_t c = run(r, cid, hint, first, reg, prog, 0, true);
		EXPECT(c.rc == 0 && c.n_rec == w.size() && c.n_sel == keep.size(), "%d: counting: rc %d, %llu of %llu", it, c.rc, (unsigned long long)c.n_sel, (unsigned long long)c.n_rec);
		if (!keep.empty()) {
			const got_t o = run(r, cid, hint, first, reg, prog, keep.size() - 1, false);
			EXPECT(o.rc == SSG_EOVERFLOW && o.n_rec == w.size() && o.n_sel == keep.size() && untouched(o), "%d: one record less of room: rc %d", it, o.rc);
		}
		ssg_recs_free(r);
	}
	if (n_fail) { fprintf(stderr, "bam_select_fuzz: %ld checks failed\n", n_fail); return 1; }
	printf("bam_select_fuzz: clean (3000 cases, %ld refused, %ld of %ld records kept)\n", n_refused, n_kept, n_seen);
	return bai_part();
}
