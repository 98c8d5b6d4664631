/*
 * devread.h -- what the executables that read a BAM file through the device's record store share (sambamba: view, index, merge, depth; bamkit: bamtofastq): the
 * file's whole BGZF members read at offsets of their own, the test of what a device read path needs, the store's holder, the words for a member the device
 * could not inflate and for a stage's refusal, the kernel times of SSG_PROF, the page-locked output buffer, the chunks of a .bai for a list of regions, and the
 * reader of a chunk list's batches into the store (dev_batches_t).  The including file defines die(const std::string&) first.
 */
#ifndef SSG_DEVREAD_H
#define SSG_DEVREAD_H
#include <cerrno>
#include <cstring>
#include <string>
#include <vector>
#include <sys/stat.h>
#include <unistd.h>
#include "../../include/ssgpu.h"
#include "bamio.h"

static void die(const std::string &m);

/* whole BGZF members of a file, read at offsets of its own (pread): a bgzf_in_t on the same descriptor is not disturbed */
struct raw_members_t {
	int fd; const char *name; uint64_t fpos, addr; bool eof; std::vector<uint8_t> buf; size_t used;   /* buf[0] lies at file offset addr; buf[0 .. used) are the members of the last next() */
	std::vector<uint64_t> moff; uint64_t inflated; bool at_end; uint64_t limit;   /* limit: no member that begins at or behind this file offset is taken (a reader of one chunk of an index) */
	raw_members_t() : fd(-1), name(""), fpos(0), addr(0), eof(false), used(0), inflated(0), at_end(false), limit(~(uint64_t)0) {}
	void start(int fd_, const char *name_, uint64_t file_off) { fd = fd_; name = name_; fpos = addr = file_off; eof = false; buf.clear(); used = 0; }
	bool fill(size_t need)
	{
		const size_t STEP = (size_t)8 << 20;
		while (buf.size() < need && !eof) {
			const size_t old = buf.size(); buf.resize(old + STEP);
			const ssize_t r = pread(fd, buf.data() + old, STEP, (off_t)fpos);
			if (r < 0) { buf.resize(old); if (errno == EINTR) continue; die(std::string("cannot read ") + name + ": " + strerror(errno)); }
			buf.resize(old + (size_t)r); fpos += (uint64_t)r;
			if (r == 0) eof = true;
		}
		return buf.size() >= need;
	}
	/* the next members: as many as inflate to at most `window' bytes -- but at least up to the first that has any -- and at most max_members; false at the end of the file */
	bool next(uint64_t window, size_t max_members)
	{
		if (used) { buf.erase(buf.begin(), buf.begin() + (ptrdiff_t)used); addr += used; used = 0; }
		moff.assign(1, 0); inflated = 0;
		size_t pos = 0;
		while (moff.size() - 1 < max_members && addr + pos < limit) {
			if (!fill(pos + 18)) { if (buf.size() > pos) die(std::string("truncated BGZF header in ") + name); break; }
			if (buf[pos] != 0x1f || buf[pos + 1] != 0x8b || buf[pos + 2] != 8 || !(buf[pos + 3] & 4)) die(std::string("not a BGZF block in ") + name);
			const size_t xlen = buf[pos + 10] | (size_t)buf[pos + 11] << 8;
			if (!fill(pos + 12 + xlen)) die(std::string("truncated BGZF header in ") + name);
			size_t bsize = 0;
			for (size_t o = 12; o + 4 <= 12 + xlen; ) { const uint8_t *h = buf.data() + pos; const size_t sl = h[o + 2] | (size_t)h[o + 3] << 8; if (h[o] == 'B' && h[o + 1] == 'C' && sl == 2 && o + 6 <= 12 + xlen) bsize = (size_t)(h[o + 4] | (size_t)h[o + 5] << 8) + 1; o += 4 + sl; }
			if (bsize < 28 || !fill(pos + bsize)) die(std::string("truncated BGZF block in ") + name);
			uint32_t isz; memcpy(&isz, buf.data() + pos + bsize - 4, 4);
			if (inflated > 0 && inflated + isz > window) break;
			pos += bsize; moff.push_back(pos); inflated += isz;
		}
		used = pos;
		at_end = addr + pos >= limit || !fill(pos + 1);   /* (nothing behind these members: the caller need not come back to learn it) */
		return moff.size() > 1;
	}
	size_t n() const { return moff.size() - 1; }
	uint64_t end_addr() const { return addr + used; }
};

struct recs_holder_t { ssg_recs_t *r; recs_holder_t() : r(0) {} ~recs_holder_t() { if (r) ssg_recs_free(r); } };
/* what the device read path needs before it starts: a device, and an input that can be read at offsets */
static bool dev_read_ready(int fd, std::string &why)
{
	if (ssg_device_count() < 1) { why = "no device"; return false; }
	struct stat sb;
	if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) { why = "an input is not a regular file"; return false; }
	return true;
}
/* ssg_recs_append_bgzf came back with SSG_EIO: the first bad member of the reader's batch, as the host readers name it */
static std::string dev_inflate_failed(const char *cmd, const raw_members_t &rd, const std::vector<int32_t> &status)
{
	const size_t nm = rd.n(); size_t k = 0;
	while (k + 1 < nm && !status[k]) ++k;
	return std::string(cmd) + ": inflate failed: BGZF member at file offset " + std::to_string(rd.addr + rd.moff[k]) + " of " + rd.name + " (device status " + std::to_string(status[k]) + ")";
}
/* a stage entry (ssg_recs_scan, ssg_recs_select, ...) came back with rc: SSG_EALIGN and SSG_EIO speak of the file, in the user's words -- the library's text without
 * its `entry' prefix ("ssg_recs_scan: "); anything else is the library's own line */
static std::string dev_stage_error(int rc, const char *file, const char *entry)
{
	return rc == SSG_EALIGN || rc == SSG_EIO ? std::string(file) + (rc == SSG_EALIGN ? " is " : ": ") + (ssg_last_error() + strlen(entry)) : std::string(ssg_last_error());
}
/* SSG_PROF=1: the device time of every kernel of the command's device path (HIP events around each launch), one line each at the end */
static void dev_prof_begin() { if (getenv("SSG_PROF")) { ssg_prof_reset(); ssg_prof_enable(1); } }
static void dev_prof_report(const char *tag, const char *cmd)
{
	if (!getenv("SSG_PROF")) return;
	const char *nm[64]; double ms[64]; long cnt[64];
	const int n = std::min(ssg_prof_get(64, nm, ms, cnt), 64);
	for (int i = 0; i < n; ++i) fprintf(stderr, "[%s] %s: kernel %-24s %9.1f ms in %ld launches\n", tag, cmd, nm[i], ms[i], cnt[i]);
}
/* page-locked host memory the device writes its output blocks or text into */
struct host_pinned_t {
	uint8_t *p; uint64_t cap;
	host_pinned_t() : p(0), cap(0) {}
	~host_pinned_t() { if (p) ssg_host_free(p); }
	bool grow(uint64_t need) { if (need <= cap) return true; if (p) ssg_host_free(p); p = (uint8_t*)ssg_host_alloc((size_t)need); cap = p ? need : 0; return p != 0; }
};
/* what the regions of `in' say to read: the chunks its .bai gives for them, sorted and merged.  The index must be there, not older than the file, and of the
 * header's n_ref references; anything else ends the program in cmd's name. */
static void bai_chunks_for(const char *cmd, const char *in, int fd, size_t n_ref, const std::vector<ssg_bam_region_t> &regions, std::vector<bai_reader_t::chunk_t> &chunks)
{
	const std::string bai = std::string(in) + ".bai", c = std::string(cmd) + ": ";
	struct stat sb, si;
	if (stat(bai.c_str(), &si) != 0) die(c + "regions need the index " + bai + ", which is not there (sambamba index)");
	if (fstat(fd, &sb) == 0 && si.st_mtime < sb.st_mtime) die(c + "the index " + bai + " is older than " + in + " (sambamba index)");
	bai_reader_t idx; std::string err;
	if (!idx.load(bai.c_str(), err)) die(c + "the index " + bai + ": " + err);
	if (idx.refs.size() != n_ref) die(c + "the index " + bai + " has " + std::to_string(idx.refs.size()) + " references, the header of " + in + " has " + std::to_string(n_ref));
	chunks.clear();
	for (const ssg_bam_region_t &r : regions) idx.query(r.tid, r.beg, r.end, chunks);
	bai_chunks_merge(chunks);
}

/* The batches of a chunk list: every chunk [u, v) of virtual offsets (one chunk (v0, ~0): the whole file from v0) is read as whole members from u >> 16 through the
 * member that holds v, at most max_members and `window' inflated bytes a batch -- and, with max_comp, max_comp compressed ones -- and each batch is inflated into the
 * store as a chunk of its own (ssg_recs_append_bgzf).  Of a batch: cid; hint[0 .. n()], the members' offsets in the chunk's stream, the last one shortened to v's
 * offset in the chunk's last member; first, where its first record begins (u & 0xffff in a chunk's first batch, 0 behind it); rd, the members themselves.
 * next(): DEV_BATCH, DEV_END, or DEV_FAIL with `why' (no command's name in it: the caller ends, fails or falls back).  A member the device could not inflate ends
 * the program here, as the host readers do.  check_first = false: a `first' behind the batch's end is the caller's to judge. */
enum { DEV_END = 0, DEV_BATCH = 1, DEV_FAIL = -1 };
struct dev_batches_t {
	const char *cmd; ssg_recs_t *recs; int fd; const char *name; std::vector<bai_reader_t::chunk_t> chunks; uint64_t window, max_comp; size_t max_members; bool check_first;
	raw_members_t rd; size_t ci; bool chunk_open; uint64_t next_first; std::vector<int32_t> status;
	uint32_t cid; std::vector<uint64_t> hint; uint64_t first; std::string why;
	dev_batches_t() : cmd(""), recs(0), fd(-1), name(""), window(0), max_comp(0), max_members(0), check_first(true), ci(0), chunk_open(false), next_first(0), cid(0), first(0) {}
	void init(const char *cmd_, ssg_recs_t *recs_, int fd_, const char *name_, uint64_t window_, size_t max_members_) { cmd = cmd_; recs = recs_; fd = fd_; name = name_; window = window_; max_members = max_members_; }
	void whole_file(uint64_t v0) { bai_reader_t::chunk_t c; c.u = v0; c.v = ~(uint64_t)0; chunks.assign(1, c); }
	size_t n() const { return rd.n(); }
	int next()
	{
		for (;;) {
			if (ci >= chunks.size()) return DEV_END;
			const bai_reader_t::chunk_t &c = chunks[ci];
			if (!chunk_open) { rd.start(fd, name, c.u >> 16); next_first = c.u & 0xffff; chunk_open = true; }
			rd.limit = c.v == ~(uint64_t)0 ? c.v : (c.v >> 16) + ((c.v & 0xffff) ? 1 : 0);
			if (max_comp && rd.end_addr() + max_comp < rd.limit) rd.limit = rd.end_addr() + max_comp;   /* (no member that begins behind this many compressed bytes; the first one always) */
			if (!rd.next(window, max_members)) { chunk_open = false; ++ci; continue; }
			const size_t nm = rd.n();
			hint.resize(nm + 1); status.assign(nm, 0);
			const int rc = ssg_recs_append_bgzf(recs, rd.buf.data(), rd.moff.data(), (long)nm, &cid, hint.data(), status.data());
			if (rc == SSG_EIO) die(dev_inflate_failed(cmd, rd, status));
			if (rc) { why = ssg_last_error(); return DEV_FAIL; }
			const bool last = (c.v & 0xffff) && rd.addr + rd.moff[nm - 1] == c.v >> 16;   /* the chunk's last member: the stream ends at v */
			const uint64_t end = last ? hint[nm - 1] + (c.v & 0xffff) : hint[nm];
			first = next_first; next_first = 0;
			if (end > hint[nm] || (check_first && first > end)) { why = std::string("the index of ") + name + " points behind a block's end"; return DEV_FAIL; }
			hint[nm] = end;
			return DEV_BATCH;
		}
	}
};
#endif
