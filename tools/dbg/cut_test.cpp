#include <stdio.h>
#include <stdlib.h>
#include <random>
#include "../../speedseq_amd/host/bamio.h"
/* cut_test -- bgzf_cut_blocks (speedseq_amd/host/bamio.h), the block cuts of the device's writers, against the writer it restates: records of the same lengths go
 * through bgzf_out_t::record into a file, and the ISIZE of every member of that file (the end-of-file marker apart) must be the difference of two neighbouring cuts.
 * With forced cuts: close_block() before those records, and force_blk[k] must be the member whose payload begins at the forced record.
 * usage: cut_test : prints the number of sequences checked; exit 1 with the first difference */
static int g_fd = -1; static std::vector<uint8_t> g_bytes; static int g_checked = 0;

/* the ISIZEs of the members bgzf_out_t writes for these records, without the end-of-file marker's */
static std::vector<uint64_t> written_isizes(const std::vector<size_t> &len, const std::vector<size_t> &force)
{
	if (ftruncate(g_fd, 0) != 0 || lseek(g_fd, 0, SEEK_SET) != 0) { perror("cut_test: temporary file"); exit(2); }
	{	bgzf_out_t o(g_fd, 0, 1); size_t fk = 0;
		for (size_t i = 0; i < len.size(); ++i) {
			for (; fk < force.size() && force[fk] <= i; ++fk) if (force[fk] == i) o.close_block();
			o.record(g_bytes.data(), len[i]);
		}
		o.finish(); }
	const off_t size = lseek(g_fd, 0, SEEK_CUR);
	std::vector<uint8_t> f((size_t)size);
	if (pread(g_fd, f.data(), f.size(), 0) != (ssize_t)f.size()) { perror("cut_test: read back"); exit(2); }
	std::vector<uint64_t> isz;
	for (size_t p = 0; p < f.size(); ) {
		if (p + 18 > f.size() || f[p] != 0x1f || f[p + 12] != 'B' || f[p + 13] != 'C') { fprintf(stderr, "cut_test: not a BGZF member at %zu\n", p); exit(1); }
		const size_t bsize = (size_t)(f[p + 16] | (size_t)f[p + 17] << 8) + 1;
		if (p + bsize > f.size()) { fprintf(stderr, "cut_test: a member runs past the file's end at %zu\n", p); exit(1); }
		uint32_t v; memcpy(&v, f.data() + p + bsize - 4, 4); isz.push_back(v); p += bsize;
	}
	if (isz.empty() || isz.back() != 0 || f.size() < 28 || memcmp(f.data() + f.size() - 28, BGZF_EOF, 28)) { fprintf(stderr, "cut_test: no end-of-file marker\n"); exit(1); }
	isz.pop_back();
	return isz;
}

static void check(const char *what, const std::vector<size_t> &len, const std::vector<size_t> *force)
{
	std::vector<uint64_t> cum(len.size() + 1, 0), cut; std::vector<size_t> blk;
	for (size_t i = 0; i < len.size(); ++i) cum[i + 1] = cum[i] + len[i];
	if (force) bgzf_cut_blocks(cum.data(), len.size(), cut, force, &blk); else bgzf_cut_blocks(cum.data(), len.size(), cut);
	const std::vector<uint64_t> isz = written_isizes(len, force ? *force : std::vector<size_t>());
	bool ok = !cut.empty() && cut[0] == 0 && cut.size() == isz.size() + 1;
	for (size_t b = 0; ok && b < isz.size(); ++b) ok = cut[b + 1] - cut[b] == isz[b];
	if (!ok) {
		fprintf(stderr, "cut_test: %s (%zu records%s): bgzf_out_t wrote %zu members, bgzf_cut_blocks cut %zu blocks\n", what, len.size(), force ? ", forced cuts" : "", isz.size(), cut.size() - 1);
		for (size_t b = 0; b < isz.size() || b + 1 < cut.size(); ++b)
			if (b >= isz.size() || b + 1 >= cut.size() || cut[b + 1] - cut[b] != isz[b]) { fprintf(stderr, "  first difference: block %zu, written %lld, cut %lld\n", b, b < isz.size() ? (long long)isz[b] : -1ll, b + 1 < cut.size() ? (long long)(cut[b + 1] - cut[b]) : -1ll); break; }
		exit(1);
	}
	if (force) {
		if (blk.size() != force->size()) { fprintf(stderr, "cut_test: %s: force_blk has %zu entries for %zu forced indices\n", what, blk.size(), force->size()); exit(1); }
		std::vector<uint64_t> start(isz.size() + 1, 0);   /* where every written member's payload begins in the stream */
		for (size_t b = 0; b < isz.size(); ++b) start[b + 1] = start[b] + isz[b];
		for (size_t k = 0; k < force->size(); ++k) {
			const size_t i = (*force)[k];
			const bool good = i >= len.size() ? blk[k] == 0 : blk[k] < isz.size() && start[blk[k]] == cum[i];
			if (!good) { fprintf(stderr, "cut_test: %s: force_blk[%zu] = %zu is not the member that begins at record %zu (stream offset %llu)\n", what, k, blk[k], i, (unsigned long long)cum[i < len.size() ? i : len.size()]); exit(1); }
		}
	}
	++g_checked;
}

int main()
{
	FILE *tmp = tmpfile(); if (!tmp) { perror("cut_test: tmpfile"); return 2; }
	g_fd = fileno(tmp);
	const size_t M = BGZF_MAX_PAYLOAD;
	g_bytes.resize(4 * M + 3); for (size_t i = 0; i < g_bytes.size(); ++i) g_bytes[i] = (uint8_t)(i * 131 + (i >> 8));
	check("empty", std::vector<size_t>(), 0);
	const size_t edge[5] = { 1, M - 1, M, M + 1, 4 * M + 3 };
	for (size_t L : edge) { check("one record", std::vector<size_t>(1, L), 0); check("between records of 200 bytes", std::vector<size_t>{ 200, L, 200 }, 0); }
	const std::vector<size_t> fills[5] = { { 200, M - 200 }, { 200, M - 200, 200 }, { 200, M - 199, 200 }, { 200, M - 201, 1, 1 }, { 100, 2 * M - 100, 100 } };   /* a record that ends where its block does, one byte short of it, one behind it */
	for (const std::vector<size_t> &l : fills) check("records that fill a block to its last byte", l, 0);
	{ std::vector<size_t> l(5000, 3); l.push_back(0xff00); check("5000 records of 3 bytes and one of a block", l, 0); }
	check("1100 records of one block each", std::vector<size_t>(1100, M), 0);   /* (across bgzf_out_t's drain at 1024 closed blocks) */
	std::mt19937_64 rng(20240607);
	for (int s = 0; s < 300; ++s) {
		std::vector<size_t> l((size_t)(1 + rng() % 300));
		for (size_t &x : l) x = rng() % 100 == 0 ? 70000 : 36 + (size_t)(rng() % 365);
		check("seeded lengths", l, 0);
		std::vector<size_t> force;
		for (int k = 0; k < 4; ++k) force.push_back((size_t)(rng() % l.size()));
		if (s % 3 == 0) force.push_back(0);
		if (s % 3 == 1) force.push_back(force[0]);          /* two equal indices */
		if (s % 5 == 0) force.push_back(l.size());          /* (behind the last record: names no block) */
		std::sort(force.begin(), force.end());
		check("seeded lengths", l, &force);
	}
	printf("cut_test: %d sequences: bgzf_cut_blocks cuts as bgzf_out_t::record\n", g_checked);
	return 0;
}
