/*
 * devread.h -- what the executables that read a BAM file through the device's record store share (sambamba: view, index, merge; bamkit: bamtofastq): the
 * file's whole BGZF members read at offsets of their own, the test of what a device read path needs, the store's holder, and the words for a member the
 * device could not inflate.  The including file defines die(const std::string&) first.
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
#endif
