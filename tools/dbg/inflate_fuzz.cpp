/*
 * inflate_fuzz.cpp -- memory safety of ssg_k_bgzf_inflate's error paths, on the host emulation and under the sanitizers (never on a GPU: a stand-alone
 * program, `make fuzz-inflate` builds and runs it).  It feeds ssg_bgzf_inflate
 *   - the malformed members of tests/test_bgzf_inflate.py (tests/golden/bgzf_inflate_malformed.bin: u32 count, then u32 length + bytes each; the test
 *     module writes the file and checks that it is current), and
 *   - 2000 seeded mutations of ten members (zlib levels 1, 6, 9, fixed code, Huffman only, RLE, stored, many blocks; four payload shapes): bit flips,
 *     byte changes, zeroed and repeated stretches, truncations with the trailer kept, other ISIZEs,
 * every one twice: alone, its device copy followed by poisoned slack (SSG_EMU_POISON), and in a batch between good neighbours.  Checked: status 0
 * exactly where zlib accepts the member (stream end reached, ISIZE bytes, CRC-32), then with zlib's bytes; the same status alone and in the batch (a
 * reader that looked past its member would see other bytes); good neighbours intact; 64 guard bytes on both sides of the output untouched.  The sanitizers
 * watch the rest: the device copies are heap blocks of the emulation.
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
static long n_fail = 0;
#define EXPECT(c, ...) do { if (!(c)) { if (++n_fail < 20) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static bytes_t payload(int shape, size_t n)
{
	bytes_t p;
	while (p.size() < n) {
		if (shape == 0) { char b[64]; const int k = snprintf(b, sizeof(b), "@r%u/1\tACGTTGCA%.*s\tIIIIHHHGG#\n", rnd() % 999, (int)(rnd() % 9), "ACGTACGTA"); p.insert(p.end(), b, b + k); }
		else if (shape == 1) { const uint8_t v = (uint8_t)rnd(); p.insert(p.end(), 1 + rnd() % 300, v); }
		else if (shape == 2) p.push_back((uint8_t)rnd());
		else { uint32_t core[9] = { 180, rnd() % 25, rnd() % 100000000u, 0x12345678u, (99u << 16) | 1u, 150, rnd() % 25, rnd() % 100000000u, 0 }; p.insert(p.end(), (uint8_t*)core, (uint8_t*)core + 36);
			for (int i = 0; i < 75; ++i) p.push_back((uint8_t)rnd());
			for (int i = 0; i < 150; ++i) p.push_back((uint8_t)("\x28\x28\x28\x25\x0c"[rnd() % 5]));
			const char *t = "NMC\0MDZ150\0RGZgrp1"; p.insert(p.end(), t, t + 19); }
	}
	p.resize(n);
	return p;
}
static bytes_t frame(const bytes_t &stream, uint32_t crc, uint32_t isize)
{
	static const uint8_t h[16] = { 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0 };
	bytes_t m(h, h + 16); const size_t total = 18 + stream.size() + 8;
	m.push_back((uint8_t)((total - 1) & 255)); m.push_back((uint8_t)((total - 1) >> 8));
	m.insert(m.end(), stream.begin(), stream.end());
	for (int i = 0; i < 4; ++i) m.push_back((uint8_t)(crc >> (8 * i)));
	for (int i = 0; i < 4; ++i) m.push_back((uint8_t)(isize >> (8 * i)));
	return m;
}
static bytes_t deflate_raw(const bytes_t &p, int level, int mem, int strategy)
{
	z_stream zs; memset(&zs, 0, sizeof(zs));
	if (deflateInit2(&zs, level, Z_DEFLATED, -15, mem, strategy) != Z_OK) abort();
	bytes_t o(p.size() + p.size() / 8 + 1024);
	zs.next_in = (Bytef*)p.data(); zs.avail_in = (uInt)p.size(); zs.next_out = o.data(); zs.avail_out = (uInt)o.size();
	if (deflate(&zs, Z_FINISH) != Z_STREAM_END) abort();
	o.resize(zs.total_out); deflateEnd(&zs);
	return o;
}
/* zlib's verdict on a member with the 18-byte header: good (and then its bytes) or not */
static bool zlib_good(const bytes_t &m, bytes_t &out)
{
	const size_t xlen = m[10] | (size_t)m[11] << 8;
	uint32_t crc, isize; memcpy(&crc, m.data() + m.size() - 8, 4); memcpy(&isize, m.data() + m.size() - 4, 4);
	out.assign((size_t)isize + 1, 0);
	z_stream zs; memset(&zs, 0, sizeof(zs));
	if (inflateInit2(&zs, -15) != Z_OK) abort();
	zs.next_in = (Bytef*)m.data() + 12 + xlen; zs.avail_in = (uInt)(m.size() - 12 - xlen - 8); zs.next_out = out.data(); zs.avail_out = (uInt)out.size();
	const int rc = inflate(&zs, Z_FINISH);
	const bool good = rc == Z_STREAM_END && zs.total_out == isize && (uint32_t)crc32(crc32(0, 0, 0), out.data(), isize) == crc;
	inflateEnd(&zs);
	out.resize(isize);
	return good;
}
static uint32_t isize_of(const bytes_t &m) { uint32_t v; memcpy(&v, m.data() + m.size() - 4, 4); return v; }

/* one call over `ms' with guards around the output; status and bytes per member */
static int run(const std::vector<bytes_t> &ms, std::vector<int32_t> &st, std::vector<bytes_t> &outs)
{
	bytes_t blob; std::vector<uint64_t> moff(1, 0); uint64_t need = 0;
	for (const bytes_t &m : ms) { blob.insert(blob.end(), m.begin(), m.end()); moff.push_back(blob.size()); need += isize_of(m); }
	bytes_t out((size_t)need + 128, 0xAB); std::vector<uint64_t> off(ms.size() + 1, 77);
	st.assign(ms.size(), -9);
	const int rc = ssg_bgzf_inflate(blob.data(), moff.data(), (long)ms.size(), out.data() + 64, need, off.data(), st.data());
	for (size_t i = 0; i < 64; ++i) EXPECT(out[i] == 0xAB && out[64 + need + i] == 0xAB, "guard byte %zu written", i);
	outs.clear();
	if (rc != 0 && rc != SSG_EIO) return rc;
	EXPECT(off[ms.size()] == need, "out_off");
	for (size_t k = 0; k < ms.size(); ++k) outs.push_back(bytes_t(out.begin() + 64 + (size_t)off[k], out.begin() + 64 + (size_t)off[k + 1]));
	return rc;
}

static void judge(const std::vector<bytes_t> &cases, const std::vector<bytes_t> &goods, const std::vector<bytes_t> &good_payloads, const char *what)
{
	/* alone: the device copy is the member and 16 bytes of poisoned slack */
	std::vector<int32_t> alone(cases.size(), -9), st; std::vector<bytes_t> outs, want(cases.size()); std::vector<char> zgood(cases.size());
	long n_good = 0;
	for (size_t i = 0; i < cases.size(); ++i) {
		zgood[i] = zlib_good(cases[i], want[i]); n_good += zgood[i];
		const int rc = run(std::vector<bytes_t>(1, cases[i]), st, outs);
		EXPECT(rc == (zgood[i] ? 0 : SSG_EIO), "%s %zu alone: rc %d, zlib says %s", what, i, rc, zgood[i] ? "good" : "bad");
		if (rc != 0 && rc != SSG_EIO) continue;
		alone[i] = st[0];
		EXPECT((st[0] == 0) == (bool)zgood[i], "%s %zu alone: status %d, zlib says %s", what, i, (int)st[0], zgood[i] ? "good" : "bad");
		EXPECT(st[0] >= 0 && st[0] <= 3, "%s %zu: status %d", what, i, (int)st[0]);
		if (st[0] == 0 && zgood[i]) EXPECT(outs[0] == want[i], "%s %zu alone: bytes differ", what, i);
	}
	/* in batches of 100, a good member on both sides of each */
	for (size_t i0 = 0; i0 < cases.size(); i0 += 100) {
		const size_t i1 = std::min(cases.size(), i0 + 100);
		std::vector<bytes_t> ms;
		for (size_t i = i0; i < i1; ++i) { ms.push_back(goods[i % goods.size()]); ms.push_back(cases[i]); }
		ms.push_back(goods[0]);
		const int rc = run(ms, st, outs);
		EXPECT(rc == 0 || rc == SSG_EIO, "%s batch at %zu: rc %d (%s)", what, i0, rc, ssg_err_msg.c_str());
		if (rc != 0 && rc != SSG_EIO) continue;
		for (size_t i = i0; i < i1; ++i) {
			const size_t k = 2 * (i - i0);
			EXPECT(st[k] == 0 && outs[k] == good_payloads[i % goods.size()], "%s %zu: the good neighbour in front, status %d", what, i, (int)st[k]);
			EXPECT(st[k + 1] == alone[i], "%s %zu: status %d in the batch, %d alone", what, i, (int)st[k + 1], (int)alone[i]);
			if (st[k + 1] == 0 && zgood[i]) EXPECT(outs[k + 1] == want[i], "%s %zu in the batch: bytes differ", what, i);
		}
		EXPECT(st.back() == 0 && outs.back() == good_payloads[0], "%s: the last good neighbour", what);
	}
	printf("%s: %zu members, %ld good by zlib's rule\n", what, cases.size(), n_good);
}

int main(int argc, char **argv)
{
	setenv("SSG_EMU_POISON", "1", 1);
	/* the ten members */
	struct { int shape; size_t n; int level, mem, strategy; } const spec[10] = {
		{ 3, 5000, 6, 8, Z_DEFAULT_STRATEGY }, { 0, 3000, 9, 8, Z_DEFAULT_STRATEGY }, { 1, 8000, 1, 8, Z_DEFAULT_STRATEGY }, { 2, 700, 6, 8, Z_DEFAULT_STRATEGY },
		{ 3, 2000, 6, 8, Z_FIXED }, { 0, 1500, 6, 8, Z_HUFFMAN_ONLY }, { 1, 4000, 6, 8, Z_RLE }, { 3, 900, 0, 8, Z_DEFAULT_STRATEGY }, { 3, 30000, 6, 1, Z_DEFAULT_STRATEGY }, { 0, 1, 6, 8, Z_DEFAULT_STRATEGY } };
	std::vector<bytes_t> goods, payloads;
	for (int k = 0; k < 10; ++k) {
		payloads.push_back(payload(spec[k].shape, spec[k].n));
		goods.push_back(frame(deflate_raw(payloads.back(), spec[k].level, spec[k].mem, spec[k].strategy), (uint32_t)crc32(crc32(0, 0, 0), payloads.back().data(), (uInt)payloads.back().size()), (uint32_t)payloads.back().size()));
	}
	judge(goods, goods, payloads, "the ten members");
	/* the malformed set of the tests */
	if (argc > 1) {
		FILE *f = fopen(argv[1], "rb"); if (!f) { perror(argv[1]); return 2; }
		uint32_t n = 0; std::vector<bytes_t> cases;
		if (fread(&n, 4, 1, f) != 1) n = 0;
		for (uint32_t i = 0; i < n; ++i) { uint32_t len; if (fread(&len, 4, 1, f) != 1 || len > 65536) { fprintf(stderr, "%s: bad file\n", argv[1]); return 2; } bytes_t m(len); if (len && fread(m.data(), 1, len, f) != len) { fprintf(stderr, "%s: short file\n", argv[1]); return 2; } cases.push_back(m); }
		fclose(f);
		if (cases.empty()) { fprintf(stderr, "%s: no members\n", argv[1]); return 2; }
		judge(cases, goods, payloads, "malformed set");
	}
	/* 2000 mutations */
	std::vector<bytes_t> muts;
	for (int it = 0; it < 2000; ++it) {
		bytes_t m = goods[(size_t)it % 10];
		const size_t s0 = 18, s1 = m.size() - 8, sn = s1 - s0;
		const int kind = (int)(rnd() % 8);
		if (kind <= 2) { const int n = 1 + (int)(rnd() % 3); for (int j = 0; j < n; ++j) { const size_t bit = rnd() % (sn * 8); m[s0 + (bit >> 3)] ^= (uint8_t)(1u << (bit & 7)); } }
		else if (kind == 3) { const int n = 1 + (int)(rnd() % 4); for (int j = 0; j < n; ++j) m[s0 + rnd() % sn] = (uint8_t)rnd(); }
		else if (kind == 4) { const size_t a = rnd() % sn, l = 1 + rnd() % 16; for (size_t j = a; j < sn && j < a + l; ++j) m[s0 + j] = (rnd() & 1) ? 0 : 0xff; }
		else if (kind == 5) { const size_t a = rnd() % sn, l = 1 + rnd() % 32; for (size_t j = a + l; j < sn && j < a + 3 * l; ++j) m[s0 + j] = m[s0 + j - l]; }
		else if (kind == 6) {   /* truncated: the first `keep' bytes of the stream, the trailer kept */
			const size_t keep = sn > 2 ? 2 + rnd() % (sn - 2) : sn;   /* (a span of at least 28 bytes) */ bytes_t s(m.begin() + (long)s0, m.begin() + (long)(s0 + keep)); uint32_t crc; memcpy(&crc, m.data() + s1, 4);
			m = frame(s, crc, isize_of(m));
		} else { const uint32_t is = isize_of(m), v = (rnd() & 1) ? (uint32_t)(rnd() % 65537) : is + (rnd() % 5) - 2; const uint32_t w = v > 65536 ? 65536 : v; memcpy(m.data() + m.size() - 4, &w, 4); if (rnd() & 1) m[s0 + rnd() % sn] ^= 0x40; }
		muts.push_back(m);
	}
	judge(muts, goods, payloads, "mutations");
	if (n_fail) { fprintf(stderr, "inflate_fuzz: %ld checks failed\n", n_fail); return 1; }
	printf("inflate_fuzz: clean\n");
	return 0;
}
