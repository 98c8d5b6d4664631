/*
 * deflate_deep_fuzz.cpp -- memory safety of ssg_k_bgzf_deflate_deep (csrc/k_bgzf_deep.h: the chain walk, the links in LDS and in scratch, the tables), on the
 * host emulation and under the sanitizers (never on a GPU: a stand-alone program, `make fuzz-deflate-deep` builds and runs it).  It feeds
 * ssg_bgzf_deflate_level at levels 7, 8 and 9
 *   - the edges of the kernel: 0, 1, 3, 4, 5 bytes; 63 / 64 / 65 (a chunk); 4095 / 4096 / 4097 (a region); 0xff00 (a full block) of records, of noise and of one
 *     byte (one chain through the whole block: the depth cap, length 258, distance 1); X + X[:32512] with 32768 random bytes X (distance 32768 is legal) and
 *     X + X[:32000] with 32769 (the only repeats lie at 32769: one of them in the stream and zlib refuses it); 300-byte records repeated with one byte
 *     changed (matches run into the chunks' ends), and
 *   - 3000 seeded payloads of five shapes (text, runs, noise, BAM-like records, a short alphabet: long chains) and lengths up to 0xff00, in batches of 40,
 * and inflates every stream with zlib: the payload comes back, the stream ends there with nothing behind it, it is at most payload + 5 bytes, 64 guard bytes
 * on both sides of the output are untouched, and a second call gives the same bytes.  Device memory comes poisoned (SSG_EMU_POISON): a link or a table entry
 * read before it is written shows as a difference or to the sanitizers, which watch every load and store -- the device buffers are heap blocks of the emulation.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <zlib.h>
#include "../../include/ssgpu.h"

thread_local std::string ssg_err_msg;      /* what ssgpu_core.cpp defines for the library */
thread_local int ssg_cur_dev = 0;
thread_local int ssg_lane = 0;

typedef std::vector<uint8_t> bytes_t;
static uint64_t rng_s = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rng_s ^= rng_s << 13; rng_s ^= rng_s >> 7; rng_s ^= rng_s << 17; return (uint32_t)(rng_s >> 16); }
static long n_fail = 0, n_streams = 0, n_stored = 0;
static uint64_t bytes_in = 0, bytes_out = 0;
#define EXPECT(c, ...) do { if (!(c)) { if (++n_fail < 20) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static bytes_t payload(int shape, size_t n)
{
	bytes_t p;
	while (p.size() < n) {
		if (shape == 0) { char b[64]; const int k = snprintf(b, sizeof(b), "@r%u/1\tACGTTGCA%.*s\tIIIIHHHGG#\n", rnd() % 999, (int)(rnd() % 9), "ACGTACGTA"); p.insert(p.end(), b, b + k); }
		else if (shape == 1) { const uint8_t v = (uint8_t)rnd(); p.insert(p.end(), 1 + rnd() % 300, v); }
		else if (shape == 2) p.push_back((uint8_t)rnd());
		else if (shape == 3) { uint32_t core[9] = { 180, rnd() % 25, rnd() % 100000000u, 0x12345678u, (99u << 16) | 1u, 150, rnd() % 25, rnd() % 100000000u, 0 }; p.insert(p.end(), (uint8_t*)core, (uint8_t*)core + 36);
			for (int i = 0; i < 75; ++i) p.push_back((uint8_t)rnd());
			for (int i = 0; i < 150; ++i) p.push_back((uint8_t)("\x28\x28\x28\x25\x0c"[rnd() % 5]));
			const char *t = "NMC\0MDZ150\0RGZgrp1"; p.insert(p.end(), t, t + 19); }
		else p.push_back((uint8_t)("ab"[(rnd() % 7) == 0]));   /* few distinct four-byte words: chains as long as the block */
	}
	p.resize(n);
	return p;
}
static bytes_t cat(const bytes_t &a, const bytes_t &b) { bytes_t r(a); r.insert(r.end(), b.begin(), b.end()); return r; }

/* one call over the blocks at a level, with guards around the output; every stream inflated */
static void run(const std::vector<bytes_t> &blocks, int level, const char *what)
{
	bytes_t pay; std::vector<uint64_t> cut(1, 0);
	for (const bytes_t &b : blocks) { pay.insert(pay.end(), b.begin(), b.end()); cut.push_back(pay.size()); }
	const uint64_t cap = pay.size() + 5 * blocks.size();
	bytes_t out[2]; std::vector<uint64_t> off[2];
	for (int pass = 0; pass < 2; ++pass) {
		out[pass].assign((size_t)cap + 128, 0xAB); off[pass].assign(blocks.size() + 1, 77);
		const int rc = ssg_bgzf_deflate_level(pay.data(), cut.data(), (long)blocks.size(), out[pass].data() + 64, cap, off[pass].data(), level);
		EXPECT(rc == 0, "%s level %d: rc %d (%s)", what, level, rc, ssg_err_msg.c_str());
		if (rc) return;
		for (size_t i = 0; i < 64; ++i) EXPECT(out[pass][i] == 0xAB && out[pass][64 + cap + i] == 0xAB, "%s level %d: guard byte %zu written", what, level, i);
	}
	EXPECT(off[0] == off[1] && out[0] == out[1], "%s level %d: the second call gave other bytes", what, level);
	for (size_t k = 0; k < blocks.size(); ++k) {
		const bytes_t &b = blocks[k];
		const size_t s0 = (size_t)off[0][k], sn = (size_t)(off[0][k + 1] - off[0][k]);
		EXPECT(off[0][k + 1] >= off[0][k] && sn <= b.size() + 5, "%s level %d block %zu: %zu bytes of stream for %zu of payload", what, level, k, sn, b.size());
		if (off[0][k + 1] < off[0][k] || off[0][k + 1] > cap) return;
		bytes_t got(b.size() + 1, 0);
		z_stream zs; memset(&zs, 0, sizeof(zs));
		if (inflateInit2(&zs, -15) != Z_OK) abort();
		zs.next_in = out[0].data() + 64 + s0; zs.avail_in = (uInt)sn; zs.next_out = got.data(); zs.avail_out = (uInt)got.size();
		const int rc = inflate(&zs, Z_FINISH);
		EXPECT(rc == Z_STREAM_END && zs.total_out == b.size() && zs.avail_in == 0, "%s level %d block %zu (%zu bytes): inflate %d (%s), %lu bytes out, %u left", what, level, k, b.size(), rc, zs.msg ? zs.msg : "", (unsigned long)zs.total_out, zs.avail_in);
		if (rc == Z_STREAM_END && zs.total_out == b.size() && !b.empty()) EXPECT(!memcmp(got.data(), b.data(), b.size()), "%s level %d block %zu: other bytes", what, level, k);
		inflateEnd(&zs);
		++n_streams; n_stored += sn == b.size() + 5; bytes_in += b.size(); bytes_out += sn;
	}
}

int main()
{
	setenv("SSG_EMU_POISON", "1", 1);
	const int levels[3] = { 7, 8, 9 };
	/* the edges */
	std::vector<bytes_t> edges;
	const size_t lens[12] = { 0, 1, 3, 4, 5, 63, 64, 65, 4095, 4096, 4097, 0xff00 };
	for (int shape = 1; shape <= 3; ++shape) for (size_t n : lens) edges.push_back(payload(shape, n));
	for (size_t n : lens) edges.push_back(bytes_t(n, 7));
	{ const bytes_t X = payload(2, 32768); edges.push_back(cat(X, bytes_t(X.begin(), X.begin() + 32512))); }
	{ const bytes_t X = payload(2, 32769); edges.push_back(cat(X, bytes_t(X.begin(), X.begin() + 32000))); }
	{	bytes_t h = payload(3, 300 * 100), r = h;   /* the second half: the records of the first, one byte changed in each */
		for (size_t k = 0; k < 100; ++k) r[k * 300 + rnd() % 300] ^= 0x55;
		edges.push_back(cat(h, r)); }
	for (int lv : levels) run(edges, lv, "edges");
	printf("edges: %zu blocks at three levels\n", edges.size());
	/* 3000 seeded payloads */
	for (int it = 0; it < 3000; it += 40) {
		std::vector<bytes_t> blocks;
		for (int k = 0; k < 40; ++k) {
			const uint32_t r = rnd() % 16;
			const size_t n = r == 0 ? 0xff00 - rnd() % 3 : r < 4 ? rnd() % 0xff01 : r < 10 ? rnd() % 9000 : rnd() % 300;
			blocks.push_back(payload((int)(rnd() % 5), n));
		}
		run(blocks, levels[(it / 40) % 3], "seeded");
	}
	printf("%ld streams inflated with zlib, %ld of them stored; %.4f of the payload\n", n_streams, n_stored, bytes_in ? (double)bytes_out / (double)bytes_in : 0.0);
	/* the levels this kernel is not asked for */
	{	const bytes_t b = payload(3, 5000); const uint64_t cut[2] = { 0, b.size() }; bytes_t o(b.size() + 5); uint64_t off[2];
		EXPECT(ssg_bgzf_deflate_level(b.data(), cut, 1, o.data(), o.size(), off, 0) == SSG_EINVAL, "level 0");
		EXPECT(ssg_bgzf_deflate_level(b.data(), cut, 1, o.data(), o.size(), off, 10) == SSG_EINVAL, "level 10");
		EXPECT(ssg_bgzf_deflate_level(b.data(), cut, 1, o.data(), o.size(), off, -1) == SSG_EINVAL, "level -1");
	}
	if (n_fail) { fprintf(stderr, "deflate_deep_fuzz: %ld checks failed\n", n_fail); return 1; }
	printf("deflate_deep_fuzz: clean\n");
	return 0;
}
