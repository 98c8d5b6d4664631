/*
 * sambamba_main.cpp -- the `sambamba` executable speedseq.config names (reference bin/speedseq.config:9), with the
 * sub-commands the reference's scripts issue:
 *   view -S -f bam [-l N] /dev/stdin          SAM text -> BAM on stdout               bin/speedseq:426,433,440,447
 *   view -H <in.bam>                          header text                             bin/speedseq:682,1032,1179
 *   view [-h] <in.bam>                        SAM text (with -h: behind the header), the lines of bam2sam.h
 *   sort -t N -m XG --tmpdir=DIR -o out <in>  coordinate sort                         bin/speedseq:427,431,434,1950
 *   index <in.bam>                            <in.bam>.bai                            bin/speedseq:486-494
 *   merge -t N out.bam in1.bam in2.bam ...    merge of coordinate-sorted files        bin/speedseq:2002-2004
 *   depth base|region|window ... <in.bam>     coverage per base, BED line or window, counted on the device (what `speedseq sv -d' and `var' ask of a BAM)
 *   stats [-F filter] [-c ..] [-i n] <in.bam> the QC report of `samtools stats', its tables counted on the device
 * Formats and orders follow the in-tree samtools / htslib 1.3.1 (bamio.h cites the lines).  Text parsing, BGZF (de)compression
 * and the gather of sorted records run on host threads; the coordinate sort itself -- a stable sort of the 64-bit keys
 * tid<<32 | (pos+1)<<1 | reverse -- runs on the MI355X through libssgpu (ssg_sort_u64_perm), chunk by chunk when the input
 * exceeds the -m budget (chunks are spilled to --tmpdir and merged; ties keep input order, as samtools' merge of sorted blocks).
 */
#include <queue>
#include <cmath>
#include <cstdarg>
#include <memory>
#include <fcntl.h>
#include <sys/stat.h>
#include "bamio.h"
#include "fastq.h"   /* chan_t */
#include "fused.h"
#include "bam2sam.h"
#include "xchg.h"
#include "ranks.h"
#include <atomic>
#include <mutex>
#include <condition_variable>
#include "../../include/ssgpu.h"

#include <time.h>
static double wall() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }
static bool dbg() { static int d = -1; if (d < 0) d = (getenv("SSG_DEBUG") || getenv("SSG_SORT_LOG")) ? 1 : 0; return d != 0; }
static int hw_threads() { unsigned n = std::thread::hardware_concurrency(); return n ? (int)std::min(n, 32u) : 4; }
static const char *g_partial_out = 0;   /* `view -o': the file being written; a command that ends in die() does not leave a part of it behind */
static void die(const std::string &m) { fprintf(stderr, "[sambamba] %s\n", m.c_str()); if (g_partial_out) unlink(g_partial_out); rk_mark_failed("sambamba"); exit(1); }   /* rank mode: the other ranks must not wait for this one */
static int open_in(const char *p) { if (!strcmp(p, "/dev/stdin") || !strcmp(p, "-")) return 0; int fd = open(p, O_RDONLY); if (fd < 0) die(std::string("cannot open ") + p); return fd; }
#include "devread.h"

/* SSG_BGZF_INFLATE_DEVICE=1 and a visible device: every reader of this process inflates its batches through ssg_bgzf_inflate (bamio.h's hook; off by
 * default).  SSG_BGZF_INFLATE_LOG=1: one line per reader at its end.  Called once, by the sub-command's thread, before its first reader is made (for
 * `sort` in the worker process). */
static void inflate_hook_setup()
{
	const char *const l = getenv("SSG_BGZF_INFLATE_LOG"); bgzf_inflate_log = l && atoi(l) != 0;
	const char *const e = getenv("SSG_BGZF_INFLATE_DEVICE");
	if (e && !strcmp(e, "1") && ssg_device_count() > 0) { bgzf_inflate_hook = ssg_bgzf_inflate; bgzf_hook_alloc = ssg_host_alloc; bgzf_hook_free = ssg_host_free; }
}

/* ---------------- view: regions ----------------
 * `name', `name:beg' and `name:beg-end' behind the file name, 1-based and inclusive, commas allowed in the numbers, as hts_parse_reg reads them: the whole string
 * is tried as a contig name first, then split at its last colon.  -L reads BED: columns 1-3, 0-based half-open; `#', `track' and `browser' lines are skipped.
 * Both become 0-based half-open (tid, beg, end); merged into one sorted list of disjoint, non-adjacent regions they are what ssg_recs_select takes, and the
 * output is their union: every record that overlaps one of them, once, in file order. */
struct hdr_name_of { const bam_hdr_t &h; hdr_name_of(const bam_hdr_t &h_) : h(h_) {} const char *operator()(int32_t t) const { return t >= 0 && t < (int32_t)h.names.size() ? h.names[(size_t)t].c_str() : "*"; } };   /* the contig names bam_record_to_sam prints */
static int view_contig(const bam_hdr_t &h, const std::string &name) { for (size_t t = 0; t < h.names.size(); ++t) if (h.names[t] == name) return (int)t; return -1; }
static bool view_number(std::string v, int64_t &x)
{
	v.erase(std::remove(v.begin(), v.end(), ','), v.end());
	if (v.empty() || v.size() > 10) return false;
	for (char c : v) if (!isdigit((unsigned char)c)) return false;
	x = strtoll(v.c_str(), 0, 10); return true;
}
static void view_region_add(const bam_hdr_t &h, const std::string &s, std::vector<ssg_bam_region_t> &out)
{
	if (s == "*") die("view: the region `*' (the reads without a contig) is not supported");
	ssg_bam_region_t r; r.beg = 0; r.end = INT32_MAX;
	r.tid = view_contig(h, s);
	if (r.tid < 0) {
		const size_t c = s.rfind(':');
		const std::string name = c == std::string::npos ? s : s.substr(0, c);
		r.tid = view_contig(h, name);
		if (r.tid < 0) die("view: unknown contig `" + name + "' in the region `" + s + "'");
		const std::string span = s.substr(c + 1); const size_t d = span.find('-');
		int64_t b = 0, e = INT32_MAX;
		if (!view_number(span.substr(0, d), b) || b < 1 || (d != std::string::npos && (!view_number(span.substr(d + 1), e) || e < b))) die("view: malformed region `" + s + "'");
		if (b > INT32_MAX) b = INT32_MAX;
		r.beg = (int32_t)(b - 1); r.end = (int32_t)std::min<int64_t>(e, INT32_MAX);
	}
	if (r.beg < r.end) out.push_back(r);
}
static void view_bed_read(const bam_hdr_t &h, const char *path, std::vector<ssg_bam_region_t> &out)
{
	FILE *f = fopen(path, "r");
	if (!f) die(std::string("cannot open ") + path);
	char line[4096]; long n = 0;
	while (fgets(line, sizeof(line), f)) {
		++n;
		char name[4096]; long long b, e;
		if (line[0] == '#' || !strncmp(line, "track", 5) || !strncmp(line, "browser", 7) || line[strspn(line, " \t\r\n")] == 0) continue;
		if (sscanf(line, "%s %lld %lld", name, &b, &e) != 3 || b < 0 || e <= b || e > INT32_MAX) die(std::string("view: malformed line ") + std::to_string(n) + " of " + path);
		ssg_bam_region_t r; r.tid = view_contig(h, name); r.beg = (int32_t)b; r.end = (int32_t)e;
		if (r.tid < 0) die(std::string("view: unknown contig `") + name + "' in line " + std::to_string(n) + " of " + path);
		out.push_back(r);
	}
	fclose(f);
}
static void view_regions_merge(std::vector<ssg_bam_region_t> &r)
{
	std::sort(r.begin(), r.end(), [](const ssg_bam_region_t &a, const ssg_bam_region_t &b) { return a.tid != b.tid ? a.tid < b.tid : a.beg != b.beg ? a.beg < b.beg : a.end < b.end; });
	size_t m = 0;
	for (size_t k = 0; k < r.size(); ++k) {
		if (m && r[m - 1].tid == r[k].tid && r[k].beg <= r[m - 1].end) r[m - 1].end = std::max(r[m - 1].end, r[k].end);   /* overlapping or adjacent */
		else r[m++] = r[k];
	}
	r.resize(m);
}
/* the region test on one record (its block_size word in front), as the kernel takes it: the last region that begins at or before the record, and its successor */
static bool view_region_keeps(const std::vector<ssg_bam_region_t> &reg, const uint8_t *rec)
{
	if (reg.empty()) return true;
	int32_t tid, pos; memcpy(&tid, rec + 4, 4); memcpy(&pos, rec + 8, 4);
	if (tid < 0) return false;
	const int32_t end = bam_endpos(rec + 4);
	size_t lo = 0, hi = reg.size();
	while (lo < hi) { const size_t mid = (lo + hi) / 2; if (reg[mid].tid < tid || (reg[mid].tid == tid && reg[mid].beg <= pos)) lo = mid + 1; else hi = mid; }
	for (size_t k = lo ? lo - 1 : 0; k < reg.size() && k <= lo; ++k) if (reg[k].tid == tid && pos < reg[k].end && end > reg[k].beg) return true;
	return false;
}

/* ---------------- view: the filter (-F) ----------------
 * A subset of sambamba's filter language, compiled by recursive descent to the postfix program of ssg_recs_select (include/ssgpu.h): the twelve flag names, six
 * integer fields with == != < <= > >= and a decimal constant, `and', `or', `not' and parentheses; `not' binds tighter than `and', `and' tighter than `or'.
 * Everything else of the language (tag filters, read_name, cigar, sequence, position, =~ ...) is refused by its token: nothing is ignored silently.  The host
 * path runs the same program with view_filter_keeps. */
struct view_filter_t {
	std::vector<std::string> tok; size_t at; std::vector<ssg_bam_fop_t> prog;
	static void refuse(const std::string &t) { die("view: filter: `" + t + "' is not supported by this filter"); }
	void tokens(const char *e)
	{
		for (const char *p = e; *p; ) {
			if (isspace((unsigned char)*p)) { ++p; continue; }
			const char *q = p;
			if (isalpha((unsigned char)*p) || *p == '_') { while (isalnum((unsigned char)*q) || *q == '_') ++q; }
			else if (isdigit((unsigned char)*p) || (*p == '-' && isdigit((unsigned char)p[1]))) { ++q; while (isdigit((unsigned char)*q)) ++q; }
			else if ((p[0] == '=' && p[1] == '=') || (p[0] == '!' && p[1] == '=') || (p[0] == '<' && p[1] == '=') || (p[0] == '>' && p[1] == '=')) q = p + 2;
			else if (*p == '<' || *p == '>' || *p == '(' || *p == ')') q = p + 1;
			else {   /* not of the subset: kept with a mark, and refused where the parser comes to it (an unsupported name in front of it is named first) */
				if (*p == '[') { while (*q && *q != ']') ++q; if (*q) ++q; }
				else q = p + ((p[0] == '=' || p[0] == '!') && p[1] == '~' ? 2 : 1);
				tok.push_back("\1" + std::string(p, q)); p = q; continue;
			}
			tok.push_back(std::string(p, q)); p = q;
		}
	}
	void emit(int op, int arg, int32_t value)
	{
		ssg_bam_fop_t f; f.op = (uint8_t)op; f.arg = (uint8_t)arg; f.pad = 0; f.value = value; prog.push_back(f);
		if (prog.size() > SSG_FOP_MAX) die("view: filter: more than " + std::to_string(SSG_FOP_MAX) + " operations");
	}
	void syntax() { if (at < tok.size() && tok[at][0] == 1) refuse(tok[at].substr(1)); die("view: filter: syntax error " + (at < tok.size() ? "at `" + tok[at] + "'" : std::string("at the end of the expression"))); }
	void primary()
	{
		static const char *const flags[12] = { "paired", "proper_pair", "unmapped", "mate_is_unmapped", "reverse_strand", "mate_is_reverse_strand", "first_of_pair", "second_of_pair",
		                                       "secondary_alignment", "failed_quality_control", "duplicate", "supplementary" };
		static const char *const fields[6] = { "mapping_quality", "ref_id", "mate_ref_id", "template_length", "sequence_length", "flag" };   /* SSG_FLD_* */
		static const char *const cmps[6] = { "==", "!=", "<", "<=", ">", ">=" };                                                              /* SSG_FOP_EQ .. */
		if (at >= tok.size()) syntax();
		const std::string t = tok[at++];
		if (t[0] == 1) refuse(t.substr(1));
		if (t == "(") { either(); if (at >= tok.size() || tok[at] != ")") die("view: filter: unbalanced parenthesis"); ++at; return; }
		if (t == "not") { primary(); emit(SSG_FOP_NOT, 0, 0); return; }
		for (int k = 0; k < 12; ++k) if (t == flags[k]) { emit(SSG_FOP_FLAG, 0, 1 << k); return; }
		for (int k = 0; k < 6; ++k) if (t == fields[k]) {
			int c = 0;
			if (at >= tok.size()) syntax();
			while (c < 6 && tok[at] != cmps[c]) ++c;
			if (c == 6) { if (tok[at][0] == 1) refuse(tok[at].substr(1)); if (tok[at] == ")" || tok[at] == "and" || tok[at] == "or") syntax(); refuse(tok[at]); }
			++at;
			if (at >= tok.size()) syntax();
			const std::string &v = tok[at];
			if (!(isdigit((unsigned char)v[0]) || v[0] == '-')) { if (isalpha((unsigned char)v[0]) || v[0] == '_') refuse(v); syntax(); }
			errno = 0; const long long x = strtoll(v.c_str(), 0, 10);
			if (errno || x < INT32_MIN || x > INT32_MAX) die("view: filter: the constant " + v + " does not fit 32 bits");
			++at; emit(SSG_FOP_EQ + c, k, (int32_t)x); return;
		}
		if (t == ")") die("view: filter: unbalanced parenthesis");
		if (t == "and" || t == "or" || !(isalpha((unsigned char)t[0]) || t[0] == '_')) { --at; syntax(); }
		refuse(t);
	}
	void both() { primary(); while (at < tok.size() && tok[at] == "and") { ++at; primary(); emit(SSG_FOP_AND, 0, 0); } }
	void either() { both(); while (at < tok.size() && tok[at] == "or") { ++at; both(); emit(SSG_FOP_OR, 0, 0); } }
	void compile(const char *e)
	{
		tokens(e); at = 0;
		if (tok.empty()) die("view: filter: an empty expression");
		either();
		if (at < tok.size()) { if (tok[at] == ")") die("view: filter: unbalanced parenthesis"); syntax(); }
	}
	view_filter_t() : at(0) {}
};
/* the program on one record (its block_size word in front), by a plain interpreter: what ssg_k_bam_select computes per lane */
static bool view_filter_keeps(const std::vector<ssg_bam_fop_t> &prog, const uint8_t *rec)
{
	if (prog.empty()) return true;
	uint32_t x[9]; memcpy(x, rec, 36);
	const int32_t field[6] = { (int32_t)(x[3] >> 8 & 0xff), (int32_t)x[1], (int32_t)x[6], (int32_t)x[8], (int32_t)x[5], (int32_t)(x[4] >> 16) };
	bool st[SSG_FOP_MAX + 1]; int d = 0;
	for (size_t pc = 0; pc < prog.size(); ++pc) {
		const ssg_bam_fop_t &f = prog[pc];
		if (f.op == SSG_FOP_FLAG) st[d++] = (field[SSG_FLD_FLAG] & f.value) != 0;
		else if (f.op == SSG_FOP_NOT) st[d - 1] = !st[d - 1];
		else if (f.op == SSG_FOP_AND) { st[d - 2] = st[d - 2] && st[d - 1]; --d; }
		else if (f.op == SSG_FOP_OR) { st[d - 2] = st[d - 2] || st[d - 1]; --d; }
		else { const int32_t v = field[f.arg], c = f.value; st[d++] = f.op == SSG_FOP_EQ ? v == c : f.op == SSG_FOP_NE ? v != c : f.op == SSG_FOP_LT ? v < c : f.op == SSG_FOP_LE ? v <= c : f.op == SSG_FOP_GT ? v > c : v >= c; }
	}
	return st[0];
}
/* the selecting form of `view' (defined behind the device read path below) */
struct view_job_t;
static void view_select_run(const char *in, int fd, bgzf_in_t *bi, bam_hdr_t &h, uint64_t v0, std::vector<ssg_bam_region_t> &reg, bool with_regions, const std::vector<ssg_bam_fop_t> &prog, bool count, bool with_hdr, bool bam_out, int level, int threads, int out_fd);

/* ---------------- view ---------------- */
static int cmd_view(int argc, char **argv)
{
	int level = -1, threads = hw_threads(); bool hdr_only = false, sam_in = false, with_hdr = false, count = false; const char *in = 0, *fmt = "sam", *expr = 0, *out_path = 0, *bed = 0; std::vector<std::string> region;
	for (int i = 0; i < argc; ++i) {
		const char *a = argv[i];
		if (!strcmp(a, "-S")) sam_in = true;
		else if (!strcmp(a, "-F") && i + 1 < argc) expr = argv[++i];
		else if (!strcmp(a, "-c")) count = true;
		else if (!strcmp(a, "-o") && i + 1 < argc) out_path = argv[++i];
		else if (!strcmp(a, "-L") && i + 1 < argc) bed = argv[++i];
		else if (!strcmp(a, "-H")) hdr_only = true;
		else if (!strcmp(a, "-h")) with_hdr = true;
		else if (!strcmp(a, "-f") && i + 1 < argc) fmt = argv[++i];
		else if (!strcmp(a, "-l") && i + 1 < argc) level = atoi(argv[++i]);
		else if (!strcmp(a, "-t") && i + 1 < argc) threads = atoi(argv[++i]);
		else if (a[0] == '-' && a[1] && strcmp(a, "-")) die(std::string("view: unsupported option ") + a);
		else region.push_back(a);
	}
	/* what stands behind the file name of a BAM input are regions (with -S, as ever, the last name is the input) */
	std::string in_name;
	if (!region.empty()) { in_name = sam_in ? region.back() : region.front(); if (sam_in) region.clear(); else region.erase(region.begin()); in = in_name.c_str(); }
	if (!in) die("usage: sambamba view [-S] [-f bam] [-l N] [-H] [-F FILTER] [-c] [-o FILE] [-L BED] <in> [region ...]");
	view_filter_t filter;
	if (expr) filter.compile(expr);
	const bool selecting = expr || count || out_path || bed || !region.empty() || (!sam_in && !hdr_only && !strcmp(fmt, "bam"));
	if (selecting && (sam_in || hdr_only || (strcmp(fmt, "sam") && strcmp(fmt, "bam")))) die("view: -F, -c, -o, -L and regions are supported for a BAM file, as SAM text, as BAM (-f bam) or as a count");
	const int fd = open_in(in);
	if (hdr_only) {
		bgzf_in_t bi(fd, 1); bam_hdr_t h;
		if (!hdr_read(bi, h)) die("view -H: not a BAM file");
		io_write_all(1, h.text.data(), h.text.size());
		return 0;
	}
	if (selecting) {   /* the records that regions and a filter keep, as SAM text, as BAM or as their number */
		bam_hdr_t h; bgzf_in_t bi(fd, threads);   /* (the reader goes on behind the header where the input cannot be read at offsets) */
		if (!hdr_read(bi, h)) die("view: not a BAM file");
		const uint64_t v0 = bi.tell();
		std::vector<ssg_bam_region_t> reg;
		for (const std::string &r : region) view_region_add(h, r, reg);
		if (bed) view_bed_read(h, bed, reg);
		view_regions_merge(reg);
		const bool with_regions = bed || !region.empty();
		int out_fd = 1;
		if (out_path) { out_fd = open(out_path, O_WRONLY | O_CREAT | O_TRUNC, 0666); if (out_fd < 0) die(std::string("cannot write ") + out_path + ": " + strerror(errno)); g_partial_out = out_path; }
		view_select_run(in, fd, &bi, h, v0, reg, with_regions, filter.prog, count, with_hdr, !strcmp(fmt, "bam"), level, threads, out_fd);
		g_partial_out = 0; if (out_path) close(out_fd);
		return 0;
	}
	if (!sam_in && !strcmp(fmt, "sam")) {   /* a BAM file as SAM text (with -h: behind its header), the lines of bam2sam.h */
		bgzf_in_t bi(fd, threads); bam_hdr_t h;
		if (!hdr_read(bi, h)) die("view: not a BAM file");
		std::string text; if (with_hdr) text = h.text;
		std::vector<uint8_t> rec;
		for (;;) {
			uint32_t bs;
			if (bi.get(&bs, 4) != 4) break;
			if (bs < 32) die("view: malformed BAM record");
			rec.resize(4 + (size_t)bs); memcpy(rec.data(), &bs, 4);
			if (bi.get(rec.data() + 4, bs) != bs) die("view: truncated BAM");
			if (!bam_record_to_sam(rec.data(), hdr_name_of(h), text)) die("view: a record with a tag type this printer does not know");
			if (text.size() > ((size_t)1 << 20)) { io_write_all(1, text.data(), text.size()); text.clear(); }
		}
		io_write_all(1, text.data(), text.size());
		return 0;
	}
	if (!sam_in || strcmp(fmt, "bam")) die("view: only `-S -f bam` (SAM text to BAM), a BAM file as SAM text, and `-H` are supported");
	/* fused stream (fused.h): the records already are BAM records; they pass through to `sambamba sort` untouched */
	char first[8]; size_t n_first = 0;
	while (n_first < 8) { ssize_t r = read(fd, first + n_first, 8 - n_first); if (r < 0) { if (errno == EINTR) continue; die("view: read error"); } if (r == 0) break; n_first += (size_t)r; }
	if (n_first == 8 && !memcmp(first, FU_MAGIC, 8)) {
		io_write_all(1, first, 8);
		std::vector<char> b((size_t)4 << 20);
		for (;;) { ssize_t r = read(fd, b.data(), b.size()); if (r < 0) { if (errno == EINTR) continue; die("view: read error"); } if (r == 0) break; io_write_all(1, b.data(), (size_t)r); }
		return 0;
	}
	bgzf_out_t out(1, level, threads);
	bam_hdr_t h; bool hdr_done = false;
	/* a reader thread cuts stdin into pieces of whole lines (the pipe from samblaster is read while the previous piece is encoded) */
	struct piece_t { std::vector<char> buf; size_t end; };
	chan_t<std::unique_ptr<piece_t> > ch(2);
	std::thread reader([&]() {
		std::vector<char> carry(first, first + n_first); bool eof = false;
		while (!eof) {
			std::unique_ptr<piece_t> P(new piece_t());
			P->buf.resize((size_t)48 << 20);
			size_t have = carry.size();
			if (have > P->buf.size() / 2) P->buf.resize(have * 2 + ((size_t)1 << 20));
			memcpy(P->buf.data(), carry.data(), have); carry.clear();
			while (!eof && have < P->buf.size()) {
				ssize_t r = read(fd, P->buf.data() + have, P->buf.size() - have);
				if (r < 0) { if (errno == EINTR) continue; die("view: read error"); }
				if (r == 0) { eof = true; break; }
				have += (size_t)r;
			}
			if (eof && have && P->buf[have - 1] != '\n') { if (have == P->buf.size()) P->buf.resize(have + 1); P->buf[have++] = '\n'; }
			size_t end = have;
			while (end > 0 && P->buf[end - 1] != '\n') --end;       /* complete lines only; the rest starts the next piece */
			carry.assign(P->buf.data() + end, P->buf.data() + have);
			P->end = end;
			if (end) ch.push(std::move(P));
		}
		ch.close();
	});
	std::unique_ptr<piece_t> P;
	while (ch.pop(P)) {
		const std::vector<char> &buf = P->buf; const size_t end = P->end;
		size_t p = 0;
		while (!hdr_done && p < end) {
			if (buf[p] != '@') { hdr_done = true; hdr_from_text(h); hdr_write(out, h); break; }
			const char *nl = (const char*)memchr(buf.data() + p, '\n', end - p);
			h.text.append(buf.data() + p, (size_t)(nl - (buf.data() + p)) + 1);
			p = (size_t)(nl - buf.data()) + 1;
		}
		if (hdr_done && p < end) {
			/* threads take byte ranges cut at line ends and encode the lines inside */
			const size_t T = (size_t)std::max(1, threads);
			std::vector<size_t> cutp(T + 1, end); cutp[0] = p;
			for (size_t t = 1; t < T; ++t) {
				size_t q = p + (end - p) * t / T;
				if (q < cutp[t - 1]) q = cutp[t - 1];
				const char *nl = q < end ? (const char*)memchr(buf.data() + q, '\n', end - q) : 0;
				cutp[t] = nl ? (size_t)(nl - buf.data()) + 1 : end;
			}
			std::vector<std::vector<uint8_t> > enc(T); std::vector<std::string> errs(T);
			parallel_for((int)T, T, [&](size_t a, size_t b, int) {
				for (size_t t = a; t < b; ++t) {
					enc[t].reserve((cutp[t + 1] - cutp[t]) * 9 / 10 + 1024);
					for (size_t q = cutp[t]; q < cutp[t + 1] && errs[t].empty(); ) {
						const char *s = buf.data() + q, *nl = (const char*)memchr(s, '\n', cutp[t + 1] - q), *e = nl;
						q = (size_t)(nl - buf.data()) + 1;
						while (e > s && e[-1] == '\r') --e;
						if (e == s) continue;
						std::string er;
						if (sam_line_to_bam(s, e, h, enc[t], er)) errs[t] = er + ": " + std::string(s, std::min<size_t>(80, (size_t)(e - s)));
					}
				}
			});
			for (auto &er : errs) if (!er.empty()) die("view: malformed SAM line (" + er + ")");
			for (auto &v : enc) out.put(v.data(), v.size());        /* records may straddle BGZF blocks (bgzf_write), as in any BAM stream */
		}
	}
	reader.join();
	if (!hdr_done) { hdr_from_text(h); hdr_write(out, h); }
	out.finish();
	return 0;
}

/* ---------------- sort ---------------- */
static void change_so(std::string &text, const char *so)
{	/* samtools bam_sort.c change_SO: @HD ... SO:<so> (added when there is no @HD line) */
	if (text.size() > 3 && !text.compare(0, 3, "@HD")) {
		size_t nl = text.find('\n'); if (nl == std::string::npos) return;
		size_t q = text.find("\tSO:");
		if (q != std::string::npos && q < nl) {
			size_t e = q + 4; while (e < text.size() && text[e] != '\n' && text[e] != '\t') ++e;
			if (text.compare(q + 4, e - q - 4, so) == 0) return;
			text.replace(q, e - q, std::string("\tSO:") + so);
		} else text.insert(nl, std::string("\tSO:") + so);
	} else text = std::string("@HD\tVN:1.3\tSO:") + so + "\n" + text;
}

/* records of the input, held in the chunks they arrived in (a fused frame, or ~64 MB assembled from the BGZF stream): nothing is
 * copied or re-allocated while the input streams in; a record is (chunk << 40 | offset of its block_size word) */
struct rec_store_t {
	std::vector<fu_buf_t> chunk; std::vector<size_t> chunk_len;        /* heap memory, or the mapped segment a fused frame arrived in (fused.h) */
	std::vector<uint64_t> loc, key, ord; uint64_t bytes;      /* ord (rank mode only): input ordinal of a record over all ranks, (batch << 28 | index in the batch) */
	rec_store_t() : bytes(0) {}
	const uint8_t *rec(size_t i) const { return chunk[(size_t)(loc[i] >> 40)].p + (loc[i] & (((uint64_t)1 << 40) - 1)); }
	void clear() { chunk.clear(); chunk_len.clear(); loc.clear(); key.clear(); ord.clear(); bytes = 0; }
	/* index the whole records of chunk c[0..len) */
	bool add_chunk(fu_buf_t c, size_t len, uint64_t ord_base = ~(uint64_t)0)
	{
		const uint64_t id = chunk.size(); const uint8_t *p = c.p; size_t o = 0; uint64_t k = 0;
		while (o + 4 <= len) { uint32_t bs; memcpy(&bs, p + o, 4); if (o + 4 + (size_t)bs > len || bs < 32) return false; loc.push_back(id << 40 | (uint64_t)o); key.push_back(bam_sort_key(p + o + 4)); if (ord_base != ~(uint64_t)0) ord.push_back(ord_base + k++); o += 4 + (size_t)bs; }
		if (o != len) return false;
		chunk.push_back(std::move(c)); chunk_len.push_back(len); bytes += len;
		return true;
	}
};

/* the whole records of a received block with the ordinals that came with them (rank mode's exchange) */
static bool add_chunk_ords(rec_store_t &S, fu_buf_t c, size_t len, const uint64_t *ords, size_t n)
{
	const size_t n0 = S.key.size();
	if (!S.add_chunk(std::move(c), len)) return false;
	if (S.key.size() - n0 != n) return false;
	S.ord.resize(n0);
	S.ord.insert(S.ord.end(), ords, ords + n);
	return true;
}

static void gpu_perm(const rec_store_t &S, std::vector<uint32_t> &perm)
{
	perm.resize(S.key.size());
	if (S.key.empty()) return;
	if (ssg_sort_u64_perm(S.key.data(), (int64_t)S.key.size(), perm.data())) die(std::string("sort: ") + ssg_last_error());
}

/* SSG_SORT_DEVICE_GATHER=1: the records go to the device while they arrive, chunk by chunk as rec_store_t holds them (ssg_recs_append; chunk k of the store is chunk k
 * there), so that write_sorted can have a kernel build each batch's payload in HBM (ssg_bgzf_compress_recs) where host threads copied record after record into a
 * page-locked block.  An uploader thread with a lane of its own takes the chunks from a queue the input thread only appends to: it never waits for the bus.  The
 * host copy stays -- the index thread reads it, and so does the host gather that takes over, with one log line, whenever this stops: the pool is full, an allocation
 * or a copy fails, a run is spilled.  The file is the same either way. */
struct dev_gather_t {
	struct item_t { const uint8_t *p; size_t len; };
	static const size_t QCAP = 1024;   /* chunks waiting for the bus (pointers: the chunks stay where they are) */
	std::mutex mu; std::condition_variable cv; std::deque<item_t> q; bool closed;
	std::thread th; std::atomic<int> failed; std::string why; bool on, said;
	ssg_recs_t *recs; size_t n_chunks; uint64_t bytes;
	dev_gather_t() : closed(false), failed(0), on(false), said(false), recs(0), n_chunks(0), bytes(0) {}
	~dev_gather_t() { stop("the sort ended"); }
	void fail(const std::string &w) { std::lock_guard<std::mutex> l(mu); if (!failed.load()) { why = w; failed = 1; } cv.notify_all(); }
	static void say_off(const std::string &w) { if (dbg()) fprintf(stderr, "[sambamba] sort: device gather off (%s): the records are gathered on the host\n", w.c_str()); }
	void start(uint64_t cap_bytes)
	{
		on = true;
		th = std::thread([this, cap_bytes]() {
			if (ssg_set_device(0) || ssg_set_lane(7) || ssg_recs_create(cap_bytes, &recs)) fail(ssg_last_error());
			for (;;) {
				item_t it;
				{ std::unique_lock<std::mutex> l(mu); cv.wait(l, [&] { return !q.empty() || closed; }); if (q.empty()) break; it = q.front(); q.pop_front(); }
				if (failed.load()) continue;
				uint32_t id = 0;
				if (ssg_recs_append(recs, it.p, (uint64_t)it.len, &id)) fail(ssg_last_error());
				else if (id != (uint32_t)n_chunks) fail("the device's chunk ids left the host's");
				else { ++n_chunks; bytes += it.len; }
			}
			if (failed.load() && recs) { ssg_recs_free(recs); recs = 0; }
		});
	}
	/* the input thread, for every chunk rec_store_t::add_chunk has accepted */
	void push(const uint8_t *p, size_t len)
	{
		if (!on || failed.load()) return;
		std::lock_guard<std::mutex> l(mu);
		if (q.size() >= QCAP) { if (!failed.load()) { why = "the uploader fell " + std::to_string(QCAP) + " chunks behind the input"; failed = 1; } }
		else { item_t it = { p, len }; q.push_back(it); }
		cv.notify_all();
	}
	void join() { { std::lock_guard<std::mutex> l(mu); closed = true; cv.notify_all(); } if (th.joinable()) th.join(); }
	/* before anything frees a chunk (a spill): the uploader is gone when this returns, and so is the store */
	void stop(const char *reason)
	{
		if (!on) return;
		fail(reason); join(); on = false;
		if (recs) { ssg_recs_free(recs); recs = 0; }
		if (!said && strcmp(reason, "the sort ended")) { said = true; say_off(why); }
	}
	/* the end of the input: the store with every chunk in it, or NULL */
	ssg_recs_t *finish()
	{
		if (!on) return 0;
		const double t0 = wall();
		join(); on = false;
		if (failed.load()) { if (!said) { said = true; say_off(why); } return 0; }
		if (dbg()) fprintf(stderr, "[sambamba] sort: device gather: %zu chunks, %.2f GB of records on the device; waited %.2f s for the uploader at the end of the input\n", n_chunks, (double)bytes / 1e9, wall() - t0);
		ssg_recs_t *r = recs; recs = 0;
		return r;
	}
};
/* the blocks of a final file are deflated on the device (write_sorted's rule, which SSG_BGZF_DEVICE=0 / 1 overrides) */
static bool bgzf_device_wanted() { const char *const bd = getenv("SSG_BGZF_DEVICE"); return !(bd && !strcmp(bd, "0")) && (bd || strcmp(ssg_backend(), "emu") != 0) && ssg_device_count() > 0; }
/* SSG_BGZF_DEVICE_LEVELS=1 (off by default): what is deflated on the device -- the final file, a run's blocks when they go there, the device merge -- is deflated at
 * the command's level (-l, else SSG_BAM_LEVEL, else 6) through the *_level entry points: 7, 8, 9 are the chained match finder of csrc/k_bgzf_deep.h, up to 6 the same
 * bytes as without the switch.  `sort' and `merge' set the level once, before anything is written. */
static int g_bgzf_dev_level = 6; static bool g_bgzf_dev_levels = false;
static void bgzf_dev_level_set(int level) { const char *const e = getenv("SSG_BGZF_DEVICE_LEVELS"); if (e && *e && strcmp(e, "0")) { g_bgzf_dev_levels = true; g_bgzf_dev_level = level < 0 ? 6 : level > 9 ? 9 : level < 1 ? 1 : level; } }
/* the end of SSG_SORT_LOG's "blocks deflated on" line with the switch on ("" without it: the line is what it was) */
static std::string bgzf_dev_level_note() { return !g_bgzf_dev_levels ? std::string() : "; device deflate level " + std::to_string(g_bgzf_dev_level) + (g_bgzf_dev_level >= 7 ? ": chained match finder (k_bgzf_deep.h)" : ": the one parse of levels 1-6 (k_bgzf.h)"); }
static int dev_bgzf_deflate(const uint8_t *p, const uint64_t *cut, long nb, uint8_t *out, uint64_t cap, uint64_t *off) { return ssg_bgzf_deflate_level(p, cut, nb, out, cap, off, g_bgzf_dev_level); }
static int dev_bgzf_compress(const uint8_t *p, const uint64_t *cut, long nb, uint8_t *out, uint64_t cap, uint64_t *off, uint32_t *crc) { return ssg_bgzf_compress_level(p, cut, nb, out, cap, off, crc, g_bgzf_dev_level); }
static int dev_bgzf_compress_recs(ssg_recs_t *r, const uint64_t *cut, long nb, uint8_t *out, uint64_t cap, uint64_t *off, uint32_t *crc) { return ssg_bgzf_compress_recs_level(r, cut, nb, out, cap, off, crc, g_bgzf_dev_level); }

/* the sorted records as a BGZF stream.  Blocks are cut exactly as bgzf_out_t::record cuts them (a record does not straddle blocks
 * unless it is larger than one); the gather of a block's records and its deflate run on the thread pool, groups of blocks are
 * written in order by the calling thread while later groups are still being compressed. */
/* <bam>.bai.ssg: "size mtime_s mtime_ns crc32(bai)" of a BAM and the index `sambamba sort` wrote with it */
static bool bai_note_make(const std::string &bam, std::string &note)
{
	struct stat sb; if (stat(bam.c_str(), &sb) != 0) return false;
	FILE *f = fopen((bam + ".bai").c_str(), "rb"); if (!f) return false;
	uLong crc = crc32(0L, Z_NULL, 0); uint8_t buf[65536]; size_t k;
	while ((k = fread(buf, 1, sizeof(buf), f)) > 0) crc = crc32(crc, buf, (uInt)k);
	fclose(f);
	char t[128]; snprintf(t, sizeof(t), "%lld %lld %ld %lu\n", (long long)sb.st_size, (long long)sb.st_mtim.tv_sec, (long)sb.st_mtim.tv_nsec, (unsigned long)crc);
	note = t; return true;
}
static void bai_note_write(const std::string &bam)
{
	std::string note; if (!bai_note_make(bam, note)) return;
	FILE *f = fopen((bam + ".bai.ssg").c_str(), "w"); if (!f) return;
	fputs(note.c_str(), f); fclose(f);
}

/* bai_path != NULL (the final file, a regular file): the .bai is written as well -- every field `sambamba index` would read back from the
 * file is in memory here -- with a note next to it (<bai>.ssg: size and mtime of the BAM, CRC of the index) that lets `sambamba index`,
 * which the reference runs right after the sort (bin/speedseq:491-495), recognise the pair as current instead of inflating the BAM again */
/* force_at != NULL (a sorted run on its way to the temporary directory, cmd_sort): no header; a block starts at each of these record
 * indices (ascending, <= n) and force_off receives the file offset of that block -- the run's segments, one per range of the genome */
/* seg != NULL (the merge of sorted runs, merge_runs): the file is written by several calls, one per stretch of the genome; the first writes the
 * header, the last the end-of-file block and the index, and the state that crosses calls lives in *seg */
struct seg_out_t {
	bool first, last;                                  /* set by the caller for each call */
	uint64_t coff;                                     /* file offset of the next block */
	std::unique_ptr<bai_t> idx; bool idx_ok;
	bool no_index;                                     /* the output cannot be sought: no index */
	uint64_t hdr_end;                                  /* file offset of the first block after the header */
	int ent_fd;                                        /* >= 0 (rank mode): every record's index entry + virtual offset in this file goes here, 24 bytes each (cmd_index_parts) */
	bool pending; int32_t p_tid, p_pos, p_end; bool p_mapped;   /* the last record of the previous stretch: its entry closes at the first record of the next */
	seg_out_t() : first(true), last(false), coff(0), idx_ok(true), no_index(false), hdr_end(0), ent_fd(-1), pending(false), p_tid(0), p_pos(0), p_end(0), p_mapped(false) {}
};
static void write_sorted(const rec_store_t &S, const std::vector<uint32_t> &perm, const bam_hdr_t &h, int fd, int level, int threads, const char *bai_path = 0,
                         const std::vector<size_t> *force_at = 0, std::vector<uint64_t> *force_off = 0, seg_out_t *seg = 0, std::vector<uint64_t> *force_uoff = 0, ssg_recs_t *recs = 0)
{
	const bool opens = !seg || seg->first, closes = !seg || seg->last;
	if (!force_at && opens) { bgzf_out_t out(fd, level, threads); hdr_write(out, h); out.drain(true); }
	off_t hdr_end = force_at ? (off_t)0 : !opens ? (off_t)seg->coff : (bai_path || seg) ? lseek(fd, 0, SEEK_CUR) : (off_t)-1;
	if (hdr_end < 0) { bai_path = 0; if (seg) { seg->no_index = true; hdr_end = 0; } }   /* a pipe: no offsets, no index (the file offsets kept in *seg then only count from the first record) */
	if (seg && seg->no_index) bai_path = 0;
	if (seg && opens) seg->hdr_end = (uint64_t)hdr_end;
	const bool want_off = bai_path || force_at || seg;
	const size_t n = perm.size();
	const int lvl = level < 0 ? 6 : level;
	const double tw0 = wall();
	/* virtual byte offsets of the sorted stream and the block cuts */
	std::vector<uint64_t> cum(n + 1); cum[0] = 0;
	parallel_for((int)std::min<size_t>((size_t)std::max(1, threads), n / 65536 + 1), n, [&](size_t a, size_t b, int) { for (size_t i = a; i < b; ++i) { uint32_t bs; memcpy(&bs, S.rec(perm[i]), 4); cum[i + 1] = 4 + (uint64_t)bs; } });
	for (size_t i = 0; i < n; ++i) cum[i + 1] += cum[i];
	std::vector<uint64_t> cut; std::vector<size_t> force_blk;   /* force_blk: the block that starts at each forced index */
	bgzf_cut_blocks(cum.data(), n, cut, force_at, &force_blk);
	const double tw1 = wall();
	const size_t nb = cut.size() - 1, GRP = 16, ng = (nb + GRP - 1) / GRP;   /* 1 MB of records per work item: a sort of a few hundred blocks still spreads over the pool, and the last items of a large one end together */
	/* Hand-over between the pool, the writer and the index thread is by atomics and short sleeps, not by one mutex + condition variable: with
	 * 256 workers waiting on one condition every notify_all of the writer woke them all to fight for the mutex (round 4's first timers:
	 * 1.98 s of deflate per worker inside 14.5 s of wall, 11.5 s of it `held back'); nobody here waits for long, so polling costs nothing. */
	struct grp_t { std::vector<uint8_t> bytes; std::vector<uint32_t> bsz; };
	std::vector<uint64_t> blk_coff(want_off ? nb + 1 : 0);      /* file offset of every block */
	std::vector<grp_t> grp(ng);
	std::unique_ptr<std::atomic<uint8_t>[]> done(new std::atomic<uint8_t>[ng ? ng : 1]);
	for (size_t g = 0; g < ng; ++g) done[g].store(0, std::memory_order_relaxed);
	std::atomic<size_t> next_write(0), next_grp(0);
	/* blocks deflated on the device: the final file of a sort at a compressing level, when there is a device (SSG_BGZF_DEVICE=0 keeps zlib on the
	 * host's threads; the host emulation of the kernels only does it on request, it is slow) */
	const char *const bd = getenv("SSG_BGZF_DEVICE");
	/* ... and the device checksums and frames them too (ssg_bgzf_compress: the payload is in HBM for the deflate anyway), so that the producers' host threads only gather.
	 * SSG_BGZF_DEVICE_CRC=0: CRC-32 by the gather threads (zlib) and framing on the host around ssg_bgzf_deflate's streams -- the same file, byte for byte (A/B runs, tests) */
	const char *const bdc = getenv("SSG_BGZF_DEVICE_CRC"); const bool dev_crc = !(bdc && !strcmp(bdc, "0"));
	/* a run's blocks by the host's zlib pool (level 1), the device left to `bwa mem', where the host has the cores for it (32 usable ones): at 200 M pairs behind a 16-core
	 * quota both ways end at 0.95-0.97 M pairs/s -- the device way slows bwa's kernels, the host way starves its threads (profiles/r06_soak_200M*.json).  SSG_SORT_RUN_DEVICE=0 / 1 decides. */
	const char *const rde = getenv("SSG_SORT_RUN_DEVICE");
	const bool run_on_host = force_at && (rde && *rde ? atoi(rde) == 0 : ssg_usable_cores() >= 32);
	const bool use_dev = lvl != 0 && nb > 0 && !run_on_host && !(bd && !strcmp(bd, "0")) && (bd || strcmp(ssg_backend(), "emu") != 0) && ssg_device_count() > 0 && GRP * 2 <= 2048 && 2048 % GRP == 0;
	/* ... and gathers them: recs holds the store's chunks in HBM (dev_gather_t: SSG_SORT_DEVICE_GATHER=1, the final in-memory write only); the sorted order goes up once --
	 * a location and an offset per record -- and a producer's batch is one call without a payload (ssg_bgzf_compress_recs).  The host's CRC-32 has no payload to read. */
	bool dev_gather = false;
	if (recs) {
		std::string why;
		if (force_at || seg) why = "not the final in-memory write";
		else if (!use_dev) why = nb ? "the blocks are not deflated on the device" : "no block to write";
		else if (!dev_crc) why = "SSG_BGZF_DEVICE_CRC=0: the host has no payload to checksum";
		else {
			std::vector<uint64_t> sloc(n);
			parallel_for((int)std::min<size_t>((size_t)std::max(1, threads), n / 65536 + 1), n, [&](size_t a, size_t b, int) { for (size_t i = a; i < b; ++i) sloc[i] = S.loc[perm[i]]; });
			if (ssg_set_device(0) || ssg_recs_order(recs, sloc.data(), cum.data(), (int64_t)n)) why = ssg_last_error(); else dev_gather = true;
		}
		if (!dev_gather) dev_gather_t::say_off(why);
	}
	size_t DEV_BATCH = 2048; { const char *e = getenv("SSG_SORT_DEV_BATCH"); if (e && atol(e) >= (long)GRP && atol(e) <= 2048 && atol(e) % (long)GRP == 0) DEV_BATCH = (size_t)atol(e); }   /* tests: several producers on several devices for a small file */
	/* every visible device deflates (SSG_SORT_DEVICES caps them): producer t works on device t mod n_dev, lane 1 + t / n_dev -- with one device three
	 * producers on three lanes as before, with N devices at least two per device; the writer and the index thread do not care who made a block */
	int n_devs = use_dev ? std::max(1, ssg_device_count()) : 1; { const char *e = getenv("SSG_SORT_DEVICES"); if (e && atoi(e) > 0) n_devs = std::min(n_devs, atoi(e)); }
	if (dev_gather) {   /* every producer on the device that holds the records */
		if (n_devs > 1 && dbg()) fprintf(stderr, "[sambamba] sort: write: %d devices visible, the records are on device 0: all producers run there\n", n_devs);
		n_devs = 1;
	}
	/* (SSG_SORT_PRODUCERS overrides; six producers on the one device -- a producer gathers and checksums on the host OR deflates on the device, never both at once --
	 * were slower than three on the 16-CPU host next to the MI355X: 1.33 vs 1.15 s for 5.1 GB, profiles/r06f_literal_sort_producers.json: the gather threads are the limit) */
	int want_prod = std::min(3 * n_devs, std::max(3, 2 * n_devs)); { const char *e = getenv("SSG_SORT_PRODUCERS"); if (e && atoi(e) > 0) want_prod = std::min(7 * n_devs, atoi(e)); }
	/* a run (force_at: written while the input still arrives and `bwa mem' works on the same device) takes little of it: one producer, batches of 512 blocks -- a
	 * wave of the deflate kernel holds 22 KB of LDS, seven of them fill a CU, and three producers' batches held the extension kernels of `bwa mem' to a third of
	 * their rate for as long as a run was written (profiles/r06_soak_200M.json) */
	if (force_at && use_dev && !getenv("SSG_SORT_DEV_BATCH")) { DEV_BATCH = 512; want_prod = 1; }
	const int n_prod = use_dev ? (int)std::max<size_t>(1, std::min<size_t>((size_t)want_prod, (nb + DEV_BATCH - 1) / DEV_BATCH)) : 0;
	/* ... and on a host with many cores next to the device, some batches stay with the host's pool (zlib): batch k of the file belongs to slot k mod (producers + host
	 * slots), a fixed rule -- the file's bytes do not depend on who was faster.  SSG_SORT_HOST_BATCHES: host slots per round (2 from 96 usable cores, 1 from 48, else 0: zlib at level 6 makes 35 MB/s a core). */
	int host_slots = 0;
	if (use_dev) { const char *e = getenv("SSG_SORT_HOST_BATCHES"); const double cores = std::min((double)threads, ssg_usable_cores()); host_slots = e && *e ? std::max(0, std::min(16, atoi(e))) : cores >= 96 ? 2 : cores >= 48 ? 1 : 0; if ((nb + DEV_BATCH - 1) / DEV_BATCH <= (size_t)n_prod) host_slots = 0; }
	const int slot_round = n_prod + host_slots;
	std::atomic<bool> host_takes_all(!use_dev);
	std::atomic<int> dev_failed(0);
	auto host_group = [&](size_t g) -> bool { return host_takes_all.load(std::memory_order_relaxed) || (int)((g * GRP / DEV_BATCH) % (size_t)slot_round) >= n_prod; };
	const int n_workers = use_dev ? (host_slots ? (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, threads), ng)) : 0)
	                              : (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, threads), ng));   /* no more threads than work items */
	const size_t window = use_dev ? (size_t)std::max(8, 2 * n_prod) * DEV_BATCH / GRP : std::max<size_t>(64, (size_t)n_workers * 8);   /* work items compressed ahead of the writer (memory bound: ~0.3 MB each) */
	auto nap = [](int us) { std::this_thread::sleep_for(std::chrono::microseconds(us)); };
	std::atomic<long> us_gather(0), us_deflate(0), us_window(0);   /* summed over the workers (SSG_DEBUG) */
	/* payload of block bk (records cut[bk] .. cut[bk+1] of the sorted stream, a record larger than a block split over several) into dst */
	auto gather_block = [&](size_t bk, uint8_t *dst) -> size_t {
		const uint64_t v0 = cut[bk], v1 = cut[bk + 1];
		size_t i = (size_t)(std::upper_bound(cum.begin(), cum.end(), v0) - cum.begin()) - 1; size_t w = 0;
		for (uint64_t v = v0; v < v1; ++i) { const uint8_t *r = S.rec(perm[i]); const uint64_t a = v - cum[i], e = std::min(cum[i + 1], v1) - cum[i]; memcpy(dst + w, r + a, (size_t)(e - a)); w += (size_t)(e - a); v = cum[i] + e; }
		return w;
	};
	auto worker = [&]() {
		std::vector<uint8_t> payload(BGZF_MAX_PAYLOAD), blk(65536);
		long my_g = 0, my_d = 0, my_w = 0;
		for (;;) {
			const size_t g = next_grp.fetch_add(1);
			if (g >= ng) break;
			if (done[g].load(std::memory_order_acquire)) continue;   /* (made on the device before it failed: see the writer's fall-back) */
			if (!host_group(g)) continue;                            /* (a batch of the device's producers) */
			bool give_up = false;   /* (the device failed while this thread waited: the writer wants every thread joined before it starts the host-only pool, which makes this group then) */
			if (g >= next_write.load(std::memory_order_acquire) + window) {
				const double t0 = wall();
				while (g >= next_write.load(std::memory_order_acquire) + window && !(give_up = dev_failed.load() && !host_takes_all.load())) nap(200);
				my_w += (long)((wall() - t0) * 1e6);
			}
			if (give_up) break;
			std::vector<uint8_t> ob; ob.reserve(GRP * (lvl ? 24576 : 65536));
			std::vector<uint32_t> bsz;
			for (size_t bk = g * GRP; bk < std::min(nb, (g + 1) * GRP); ++bk) {
				const double t0 = wall();
				const size_t w = gather_block(bk, payload.data());
				const double t1 = wall();
				const size_t k = bgzf_make_block(payload.data(), w, lvl, blk.data());
				ob.insert(ob.end(), blk.data(), blk.data() + k); bsz.push_back((uint32_t)k);
				my_g += (long)((t1 - t0) * 1e6); my_d += (long)((wall() - t1) * 1e6);
			}
			grp[g].bytes.swap(ob); grp[g].bsz.swap(bsz);
			done[g].store(1, std::memory_order_release);
		}
		us_gather += my_g; us_deflate += my_d; us_window += my_w;
	};
	/* ... or the blocks are made on the device (ssg_bgzf_compress; k_bgzf.h, k_bgzf_frame.h): a few producer threads, each with a stream of its own, take
	 * batches of 2048 blocks in turn -- gather into page-locked memory by host threads; deflate, CRC-32 and framing (BGZF header, CRC, ISIZE) on the
	 * GPU -- and hand the groups to the same in-order writer.  The host's cores, which the deflate of a whole genome's records kept busy
	 * for longer than the alignment took, only copy (with SSG_BGZF_DEVICE_CRC=0 they checksum and frame as well, around ssg_bgzf_deflate). */
	std::atomic<long> dev_batches(0); const long fail_after = getenv("SSG_BGZF_FAIL_AFTER") ? atol(getenv("SSG_BGZF_FAIL_AFTER")) : -1;   /* tests: the device "fails" from its n-th batch on */
	/* device gather: no gatherer thread, no payload slots -- a batch is its cuts; only the output block remains */
	auto producer_recs = [&](int t) {
		if (ssg_set_device(0) || ssg_set_lane(1 + t % 7)) { dev_failed = 1; return; }
		const int gth = std::max(1, threads / std::max(1, n_prod));
		const uint64_t O_cap = (uint64_t)DEV_BATCH * (BGZF_MAX_PAYLOAD + 31) + 64;
		uint8_t *O = (uint8_t*)ssg_host_alloc(O_cap);
		std::vector<uint64_t> off(DEV_BATCH + 1);
		long my_d = 0, my_w = 0;
		for (size_t b0 = (size_t)t * DEV_BATCH; O && b0 < nb && !dev_failed.load(); b0 += (size_t)slot_round * DEV_BATCH) {
			const size_t b1 = std::min(nb, b0 + DEV_BATCH), n_b = b1 - b0, g0 = b0 / GRP, g1 = (b1 + GRP - 1) / GRP;
			if (g0 >= next_write.load(std::memory_order_acquire) + window) { const double t0 = wall(); while (g0 >= next_write.load(std::memory_order_acquire) + window && !dev_failed.load()) nap(200); my_w += (long)((wall() - t0) * 1e6); }
			if (dev_failed.load()) break;
			const double t1 = wall();
			if ((fail_after >= 0 && dev_batches.fetch_add(1) >= fail_after) || dev_bgzf_compress_recs(recs, &cut[b0], (long)n_b, O, O_cap, off.data(), 0)) {
				fprintf(stderr, "[sambamba] sort: BGZF deflate on the device failed: %s\n", fail_after >= 0 ? "(SSG_BGZF_FAIL_AFTER: test)" : ssg_last_error()); dev_failed = 1; break; }
			const double t2 = wall();
			parallel_for((int)std::min<size_t>((size_t)std::min(gth, 8), g1 - g0), g1 - g0, [&](size_t a, size_t e, int) {
				for (size_t g = g0 + a; g < g0 + e; ++g) {   /* the members arrive framed: a group is one stretch of them */
					std::vector<uint8_t> ob; std::vector<uint32_t> bsz;
					const size_t i0 = g * GRP - b0, i1 = std::min(nb, (g + 1) * GRP) - b0;
					ob.assign(O + off[i0], O + off[i1]);
					for (size_t i = i0; i < i1; ++i) bsz.push_back((uint32_t)(off[i + 1] - off[i]));
					grp[g].bytes.swap(ob); grp[g].bsz.swap(bsz);
					done[g].store(1, std::memory_order_release);
				}
			});
			my_d += (long)((t2 - t1) * 1e6);
		}
		if (!O) dev_failed = 1;
		ssg_host_free(O);
		us_deflate += my_d; us_window += my_w;
	};
	auto producer = [&](int t) {
		if (dev_gather) { producer_recs(t); return; }
		if (ssg_set_device(t % n_devs) || ssg_set_lane(1 + (t / n_devs) % 7)) { dev_failed = 1; return; }
		const int gth = std::max(1, threads / std::max(1, n_prod));
		/* two slots: a helper thread gathers and checksums batch k + 1 on the host while this one has batch k deflated on the device (until round 6 a producer did one
		 * after the other, and the device waited whenever all producers were gathering: 0.74 s of 1.15 s for 5.1 GB, profiles/r06f_literal_sort_producers.json) */
		struct slot_t { uint8_t *P; std::vector<uint64_t> rel; std::vector<uint32_t> crc; size_t b0, n_b; std::atomic<int> state; slot_t() : P(0), b0(0), n_b(0), state(0) {} };   /* state: 0 free, 1 gathered, 2 no more batches */
		slot_t slot[2];
		for (slot_t &sl : slot) { sl.P = (uint8_t*)ssg_host_alloc(DEV_BATCH * BGZF_MAX_PAYLOAD + 64); sl.rel.resize(DEV_BATCH + 1); sl.crc.resize(DEV_BATCH); }
		const uint64_t O_cap = (uint64_t)DEV_BATCH * (BGZF_MAX_PAYLOAD + 31) + 64;   /* ssg_bgzf_bound: 5 of a stored block, 26 of the framing */
		uint8_t *O = (uint8_t*)ssg_host_alloc(O_cap);
		std::vector<uint64_t> off(DEV_BATCH + 1);
		std::atomic<long> my_g(0); long my_d = 0; std::atomic<long> my_w(0);
		const bool mem_ok = slot[0].P && slot[1].P && O;
		std::thread gatherer([&]() {
			int k = 0;
			for (size_t b0 = (size_t)t * DEV_BATCH; b0 < nb && mem_ok && !dev_failed.load(); b0 += (size_t)slot_round * DEV_BATCH, k ^= 1) {
				slot_t &sl = slot[k];
				while (sl.state.load(std::memory_order_acquire) != 0 && !dev_failed.load()) nap(100);
				const size_t b1 = std::min(nb, b0 + DEV_BATCH), n_b = b1 - b0, g0 = b0 / GRP;
				if (g0 >= next_write.load(std::memory_order_acquire) + window) { const double t0 = wall(); while (g0 >= next_write.load(std::memory_order_acquire) + window && !dev_failed.load()) nap(200); my_w += (long)((wall() - t0) * 1e6); }
				if (dev_failed.load()) break;   /* (the writer is waiting for the producers to stop before it hands the rest to the host's pool) */
				const double t0 = wall();
				for (size_t i = 0; i <= n_b; ++i) sl.rel[i] = cut[b0 + i] - cut[b0];
				parallel_for((int)std::min<size_t>((size_t)gth, n_b / 8 + 1), n_b, [&](size_t a, size_t e, int) {
					for (size_t i = a; i < e; ++i) { const size_t w = gather_block(b0 + i, sl.P + sl.rel[i]); if (!dev_crc) sl.crc[i] = (uint32_t)crc32(crc32(0L, Z_NULL, 0), sl.P + sl.rel[i], (uInt)w); }
				});
				my_g += (long)((wall() - t0) * 1e6);
				sl.b0 = b0; sl.n_b = n_b;
				sl.state.store(1, std::memory_order_release);
			}
			for (int j = 0; j < 2; ++j, k ^= 1) {   /* the end: in the slot order the consumer follows */
				slot_t &sl = slot[k];
				while (sl.state.load(std::memory_order_acquire) != 0 && !dev_failed.load()) nap(100);
				if (dev_failed.load()) break;
				sl.state.store(2, std::memory_order_release);
			}
		});
		for (int k = 0; mem_ok; k ^= 1) {
			slot_t &sl = slot[k];
			int st;
			while ((st = sl.state.load(std::memory_order_acquire)) == 0 && !dev_failed.load()) nap(50);
			if (st != 1) break;
			const size_t b0 = sl.b0, n_b = sl.n_b, b1 = b0 + n_b, g0 = b0 / GRP, g1 = (b1 + GRP - 1) / GRP;
			const double t1 = wall();
			if ((fail_after >= 0 && dev_batches.fetch_add(1) >= fail_after) || (dev_crc ? dev_bgzf_compress(sl.P, sl.rel.data(), (long)n_b, O, O_cap, off.data(), 0) : dev_bgzf_deflate(sl.P, sl.rel.data(), (long)n_b, O, O_cap, off.data()))) {
				fprintf(stderr, "[sambamba] sort: BGZF deflate on the device failed: %s\n", fail_after >= 0 ? "(SSG_BGZF_FAIL_AFTER: test)" : ssg_last_error()); dev_failed = 1; break; }
			const double t2 = wall();
			parallel_for((int)std::min<size_t>((size_t)std::min(gth, 8), g1 - g0), g1 - g0, [&](size_t a, size_t e, int) {
				static const uint8_t hdr[16] = { 0x1f,0x8b,0x08,0x04,0,0,0,0,0,0xff,0x06,0,0x42,0x43,0x02,0 };
				for (size_t g = g0 + a; g < g0 + e; ++g) {
					std::vector<uint8_t> ob; std::vector<uint32_t> bsz;
					if (dev_crc) {   /* the members arrive framed: a group is one stretch of them */
						const size_t i0 = g * GRP - b0, i1 = std::min(nb, (g + 1) * GRP) - b0;
						ob.assign(O + off[i0], O + off[i1]);
						for (size_t i = i0; i < i1; ++i) bsz.push_back((uint32_t)(off[i + 1] - off[i]));
					} else for (size_t bk = g * GRP; bk < std::min(nb, (g + 1) * GRP); ++bk) {
						const size_t i = bk - b0, clen = (size_t)(off[i + 1] - off[i]), bsize = 18 + clen + 8, at = ob.size();
						ob.resize(at + bsize);
						uint8_t *d = ob.data() + at;
						memcpy(d, hdr, 16); d[16] = (uint8_t)((bsize - 1) & 0xff); d[17] = (uint8_t)((bsize - 1) >> 8);
						memcpy(d + 18, O + off[i], clen);
						const uint32_t isz = (uint32_t)(sl.rel[i + 1] - sl.rel[i]);
						memcpy(d + 18 + clen, &sl.crc[i], 4); memcpy(d + 18 + clen + 4, &isz, 4);
						bsz.push_back((uint32_t)bsize);
					}
					grp[g].bytes.swap(ob); grp[g].bsz.swap(bsz);
					done[g].store(1, std::memory_order_release);
				}
			});
			my_d += (long)((t2 - t1) * 1e6);
			sl.state.store(0, std::memory_order_release);
		}
		if (!mem_ok) dev_failed = 1;
		gatherer.join();
		for (slot_t &sl : slot) ssg_host_free(sl.P);
		ssg_host_free(O);
		us_gather += my_g.load(); us_deflate += my_d; us_window += my_w.load();
	};
	/* the index `sambamba index` would make of this file (cmd_index below: same bai_t calls, same virtual offsets), built by a thread of
	 * its own that follows the writer: a record's virtual offset is known as soon as the group holding its block has its file offset */
	struct ent_t { int32_t tid, pos, end; uint8_t mapped; };
	const bool want_ent = bai_path || (seg && seg->ent_fd >= 0);
	std::vector<ent_t> ent(want_ent ? n : 0);
	/* the record view the index needs (position, end, mapped): made next to the producers' first batches, not before them (0.19 s of 16 M records during which the device waited) */
	auto make_ent = [&]() { if (want_ent) parallel_for((int)std::min<size_t>((size_t)std::max(1, threads / 2), n / 65536 + 1), n, [&](size_t a, size_t b, int) {
		for (size_t i = a; i < b; ++i) { const uint8_t *r = S.rec(perm[i]) + 4; bam_core_t c; memcpy(&c, r, 32); ent[i].tid = c.tid; ent[i].pos = c.pos; ent[i].end = bam_endpos(r); ent[i].mapped = !((c.flag_nc >> 16) & 4); }
	}); };
	std::thread t_ent; std::atomic<bool> ent_ready(false);
	if (bai_path && want_ent) t_ent = std::thread([&]() { make_ent(); ent_ready.store(true, std::memory_order_release); }); else { make_ent(); ent_ready.store(true); }
	struct ent_join_t { std::thread &t; ~ent_join_t() { if (t.joinable()) t.join(); } } ent_join = { t_ent };
	std::atomic<size_t> blocks_placed(0);                       /* blk_coff[0 .. blocks_placed) are final */
	std::atomic<uint64_t> file_end_v(0);                        /* virtual offset of the end of the file, 0 until the last block is placed */
	bai_t idx_own((int)h.names.size(), 0); bool idx_ok = seg ? seg->idx_ok : true; double t_idx_wait = 0;
	std::thread t_idx;
	if (bai_path) t_idx = std::thread([&]() {
		while (!ent_ready.load(std::memory_order_acquire)) nap(100);
		size_t bk = 0;
		auto wait_blocks = [&](size_t need) { if (blocks_placed.load(std::memory_order_acquire) >= need) return; const double t0 = wall(); while (blocks_placed.load(std::memory_order_acquire) < need) nap(100); t_idx_wait += wall() - t0; };
		auto voff = [&](size_t i) -> uint64_t { while (cut[bk + 1] <= cum[i]) ++bk; wait_blocks(bk + 1); return blk_coff[bk] << 16 | (cum[i] - cut[bk]); };
		auto end_of_file = [&]() -> uint64_t { wait_blocks(nb + 1); return file_end_v.load(); };
		if (!idx_ok) return;
		if (!n && !closes) return;                                     /* a stretch without records: nothing to say yet */
		bai_t *ix = &idx_own;
		if (!seg) idx_own = bai_t((int)h.names.size(), n ? voff(0) : end_of_file());
		else { if (!seg->idx) seg->idx.reset(new bai_t((int)h.names.size(), n ? voff(0) : end_of_file())); ix = seg->idx.get(); }
		if (seg && seg->pending && n) { if (ix->push(seg->p_tid, seg->p_pos, seg->p_end, voff(0), seg->p_mapped) < 0) { idx_ok = false; return; } seg->pending = false; }
		for (size_t i = 0; i < n; ++i) {
			if (i + 1 == n && !closes) { seg->pending = true; seg->p_tid = ent[i].tid; seg->p_pos = ent[i].pos; seg->p_end = ent[i].end; seg->p_mapped = ent[i].mapped != 0; break; }
			const uint64_t after = i + 1 < n ? voff(i + 1) : end_of_file();
			if (ix->push(ent[i].tid, ent[i].pos, ent[i].end, after, ent[i].mapped != 0) < 0) { idx_ok = false; break; }   /* cannot happen on a sorted stream; `sambamba index` will say so */
		}
		if (idx_ok && closes && seg && seg->pending) { if (ix->push(seg->p_tid, seg->p_pos, seg->p_end, end_of_file(), seg->p_mapped) < 0) idx_ok = false; seg->pending = false; }
		if (idx_ok && closes) ix->finish(end_of_file());
	});
	std::vector<std::thread> th;
	const double tw_spawn0 = wall();
	for (int t = 0; t < n_workers; ++t) th.emplace_back(worker);
	for (int t = 0; t < n_prod; ++t) th.emplace_back(producer, t);
	uint64_t coff = (uint64_t)(hdr_end > 0 ? hdr_end : 0);
	bool fell_back = false;
	double t_wr_wait = 0, t_wr_io = 0; const double tw_spawn = wall();
	for (size_t g = 0; g < ng; ++g) {
		if (!done[g].load(std::memory_order_acquire)) {
			const double t0 = wall();
			while (!done[g].load(std::memory_order_acquire)) {
				if (dev_failed.load() && !fell_back) {   /* a device that cannot be set up, runs out of memory or loses a kernel does not end the sort: the producers stop, the host's pool (zlib, as SSG_BGZF_DEVICE=0) makes the groups that are not there yet */
					for (auto &x : th) x.join();
					th.clear(); fell_back = true; host_takes_all = true; next_grp = 0;
					fprintf(stderr, "[sambamba] sort: compressing the rest of the output on the host (zlib level %d)\n", lvl);
					const int nw = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, threads), ng));
					for (int t = 0; t < nw; ++t) th.emplace_back(worker);
				}
				nap(50);
			}
			t_wr_wait += wall() - t0;
		}
		std::vector<uint8_t> ob; std::vector<uint32_t> bsz; ob.swap(grp[g].bytes); bsz.swap(grp[g].bsz);
		{ const double t0 = wall(); io_write_all(fd, ob.data(), ob.size()); t_wr_io += wall() - t0; }
		if (want_off) for (size_t k = 0; k < bsz.size(); ++k) { blk_coff[g * GRP + k] = coff; coff += bsz[k]; }
		next_write.store(g + 1, std::memory_order_release);
		if (bai_path) blocks_placed.store(std::min(nb, (g + 1) * GRP), std::memory_order_release);
	}
	for (auto &x : th) x.join();
	if (t_ent.joinable()) t_ent.join();
	if (force_at) {   /* a run: no end-of-file block; the offsets of its segments (indices at n = the end of the data) */
		blk_coff[nb] = coff;
		force_off->resize(force_at->size());
		for (size_t k = 0; k < force_at->size(); ++k) (*force_off)[k] = (*force_at)[k] >= n ? coff : blk_coff[force_blk[k]];
		if (force_uoff) { force_uoff->resize(force_at->size()); for (size_t k = 0; k < force_at->size(); ++k) (*force_uoff)[k] = cum[std::min((*force_at)[k], n)]; }
		return;
	}
	if (closes) io_write_all(fd, BGZF_EOF, 28);
	const double tw2 = wall();
	if (dbg() && !seg) fprintf(stderr, "[sambamba] sort: write: offsets and block cuts %.2f s, gather + deflate + write of %zu blocks %.2f s (record view for the index %.2f s, %d workers started in %.2f s; writer: waited %.2f s for blocks, wrote for %.2f s; "
	                   "per worker: gather %.2f s, deflate %.2f s, held back by the writer's window %.2f s)\n", tw1 - tw0, nb, tw2 - tw1, tw_spawn0 - tw1, n_workers, tw_spawn - tw_spawn0, t_wr_wait, t_wr_io,
	                   us_gather / 1e6 / std::max(1, n_workers + n_prod), us_deflate / 1e6 / std::max(1, n_workers + n_prod), us_window / 1e6 / std::max(1, n_workers + n_prod));
	if (dbg() && use_dev && !seg) fprintf(stderr, "[sambamba] sort: write: blocks deflated on %d device(s) (%d producer threads; %s)%s%s%s\n", n_devs, n_prod,
	                                    dev_gather ? "`gather' = nothing, `deflate' = gather, deflate, CRC-32 and framing kernels + download: the payload is built in HBM" :
	                                    dev_crc ? "`gather' = gather on the host, `deflate' = upload + kernels + download: CRC-32 on the device, framing too" : "`gather' = gather + CRC-32 on the host, `deflate' = upload + kernels + download, then framing on the host",
	                                    host_slots ? (std::string("; ") + std::to_string(host_slots) + " of every " + std::to_string(slot_round) + " batches by the host's pool (zlib)").c_str() : "",
	                                    dev_gather ? "; gather on the device" : "; gather on the host", bgzf_dev_level_note().c_str());
	if (seg) seg->coff = coff;
	if (seg && seg->ent_fd >= 0 && n) {   /* rank mode: what the index of the joined file needs of this stretch */
		std::vector<uint8_t> eb(24 * n); size_t bk = 0;
		for (size_t i = 0; i < n; ++i) {
			while (cut[bk + 1] <= cum[i]) ++bk;
			const uint64_t v = blk_coff[bk] << 16 | (cum[i] - cut[bk]);
			uint8_t *d = eb.data() + 24 * i; const uint32_t m = ent[i].mapped;
			memcpy(d, &ent[i].tid, 4); memcpy(d + 4, &ent[i].pos, 4); memcpy(d + 8, &ent[i].end, 4); memcpy(d + 12, &m, 4); memcpy(d + 16, &v, 8);
		}
		io_write_all(seg->ent_fd, eb.data(), eb.size());
	}
	if (!bai_path) return;
	blk_coff[nb] = coff;
	if (closes) { file_end_v.store((coff + 28) << 16); blocks_placed.store(nb + 1, std::memory_order_release); }
	t_idx.join();
	if (seg) seg->idx_ok = idx_ok;
	if (!idx_ok || !closes) return;
	(seg ? *seg->idx : idx_own).save(bai_path);
	if (dbg() && !seg) fprintf(stderr, "[sambamba] sort: write: index finished %.2f s after the last block (its thread waited %.2f s for block offsets)\n", wall() - tw2, t_idx_wait);
}

struct merge_src_t {   /* one coordinate-sorted BAM being merged */
	int fd; std::unique_ptr<bgzf_in_t> in; bam_hdr_t h; std::vector<uint8_t> rec; uint64_t key; bool ok;
	bool next() { uint32_t bs; if (in->get(&bs, 4) != 4) { ok = false; return false; } rec.resize(4 + (size_t)bs); memcpy(rec.data(), &bs, 4); if (in->get(rec.data() + 4, bs) != bs) die("merge: truncated BAM"); key = bam_sort_key(rec.data() + 4); ok = true; return true; }
};
static void kway_merge(std::vector<merge_src_t> &src, bgzf_out_t &out)
{	/* smallest key first; equal keys in source order (samtools bam_sort.c:1347-1375 heap order) */
	typedef std::pair<uint64_t, size_t> ent_t;
	std::priority_queue<ent_t, std::vector<ent_t>, std::greater<ent_t> > pq;
	for (size_t i = 0; i < src.size(); ++i) if (src[i].next()) pq.push(ent_t(src[i].key, i));
	while (!pq.empty()) {
		const size_t i = pq.top().second; pq.pop();
		out.record(src[i].rec.data(), src[i].rec.size());
		if (src[i].next()) pq.push(ent_t(src[i].key, i));
	}
}

/* ---- sorted runs in the temporary directory (input larger than -m allows in memory) ----
 * A run is written in segments, one per range of the genome (the ranges are fixed from the header's contig lengths before the first
 * run is written), each starting at a BGZF block of its own whose file offset is kept.  The final pass then is not one k-way merge
 * over whole runs -- a single thread moving every record -- but an independent small merge per range, run by the pool, each inflating
 * only its own byte range of every run and compressing its own stretch of the output; a writer puts the stretches out in order.  Ties
 * keep input order: equal keys share a range, and within a range the earlier run wins. */
struct run_t { std::string path; int fd; std::vector<uint64_t> seg, useg, rcnt; int ord_fd; run_t() : fd(-1), ord_fd(-1) {} };   /* rcnt / ord_fd (rank mode): records before each range; the run's ordinals, 8 bytes a record */   /* seg[g] .. seg[g + 1]: the run's records of range g in the file; useg: the same in record bytes */

static void make_ranges(const bam_hdr_t &h, size_t G, std::vector<uint64_t> &lo)
{	/* lo[g] = smallest sort key of range g (equal shares of the genome's length); reads without a position sort last: the last range */
	lo.assign(1, 0);
	uint64_t L = 0; for (int32_t l : h.lens) L += (uint64_t)(l > 0 ? l : 0);
	if (G < 2 || !L) return;
	size_t tid = 0; uint64_t base = 0;
	for (size_t g = 1; g < G; ++g) {
		const uint64_t X = (uint64_t)((unsigned __int128)L * g / G);
		while (tid < h.lens.size() && base + (uint64_t)std::max(h.lens[tid], 0) <= X) { base += (uint64_t)std::max(h.lens[tid], 0); ++tid; }
		if (tid >= h.lens.size()) break;
		const uint64_t key = (uint64_t)tid << 32 | (uint64_t)(uint32_t)((X - base + 1) << 1);
		if (key > lo.back()) lo.push_back(key);
	}
}

/* The merge of the runs is the in-memory sort again, a stretch of the genome at a time: consecutive ranges whose records -- of all runs -- fit
 * a third of the budget are read back (every BGZF block of a run's byte range inflated by the pool), indexed per (run, range) piece in
 * parallel, ordered by the device's stable radix sort of the keys (the pieces of one run are in order already, earlier runs come first:
 * ties keep input order) and written through write_sorted's pipeline -- gather on the host, deflate on the device, one in-order writer, the
 * .bai following it -- while the loader thread already inflates the next stretch. */
static void load_stretch(std::vector<run_t> &runs, size_t g0, size_t g1, int threads, rec_store_t &S)
{
	S.clear();
	struct piece_t { size_t chunk, run, g; uint64_t a, b; std::vector<uint64_t> loc, key; };
	std::vector<piece_t> pieces;
	for (size_t r = 0; r < runs.size(); ++r) {
		const run_t &R = runs[r];
		const uint64_t c0 = R.seg[g0], c1 = R.seg[g1], u0 = R.useg[g0], u1 = R.useg[g1];
		if (u1 == u0) continue;
		std::vector<uint8_t> raw((size_t)(c1 - c0));
		{	/* the byte range, read by several threads (page cache or disk) */
			const size_t PIECE = (size_t)8 << 20, np = (raw.size() + PIECE - 1) / PIECE;
			parallel_for((int)std::min<size_t>((size_t)std::max(1, threads), np), np, [&](size_t a, size_t b, int) {
				for (size_t k = a; k < b; ++k) {
					const size_t lo = k * PIECE, want = std::min(PIECE, raw.size() - lo);
					for (size_t got = 0; got < want; ) { const ssize_t q = pread(R.fd, raw.data() + lo + got, want - got, (off_t)(c0 + lo + got)); if (q < 0 && errno == EINTR) continue; if (q <= 0) die("sort: cannot read a sorted run back"); got += (size_t)q; }
				}
			});
		}
		struct blk_t { size_t at, bsize, xlen; uint64_t uo; uint32_t isz; };
		std::vector<blk_t> blk; uint64_t uo = 0;
		for (size_t o = 0; o < raw.size(); ) {
			const uint8_t *b = raw.data() + o;
			if (o + 18 > raw.size() || b[0] != 0x1f || b[1] != 0x8b || !(b[3] & 4) || b[12] != 'B' || b[13] != 'C') die("sort: a sorted run is damaged");
			blk_t k; k.at = o; k.bsize = (size_t)(b[16] | (size_t)b[17] << 8) + 1; k.xlen = b[10] | (size_t)b[11] << 8;
			if (o + k.bsize > raw.size() || k.bsize < 12 + k.xlen + 8) die("sort: a sorted run is damaged");
			memcpy(&k.isz, b + k.bsize - 4, 4); k.uo = uo; uo += k.isz; o += k.bsize;
			blk.push_back(k);
		}
		if (uo != u1 - u0) die("sort: a sorted run is damaged");
		fu_buf_t buf; if (!buf.heap((size_t)uo)) die("sort: out of memory");
		parallel_for((int)std::min<size_t>((size_t)std::max(1, threads), blk.size() / 4 + 1), blk.size(), [&](size_t a, size_t b, int) {
			z_stream zs; memset(&zs, 0, sizeof(zs));
			if (inflateInit2(&zs, -15) != Z_OK) die("sort: zlib");
			for (size_t k = a; k < b; ++k) {
				const blk_t &B = blk[k];
				if (!B.isz) continue;
				zs.next_in = (Bytef*)(raw.data() + B.at + 12 + B.xlen); zs.avail_in = (uInt)(B.bsize - 12 - B.xlen - 8); zs.next_out = buf.p + B.uo; zs.avail_out = B.isz;
				if (inflateReset(&zs) != Z_OK || inflate(&zs, Z_FINISH) != Z_STREAM_END || zs.avail_out) die("sort: a sorted run does not inflate");
			}
			inflateEnd(&zs);
		});
		const size_t id = S.chunk.size();
		for (size_t g = g0; g < g1; ++g) if (R.useg[g + 1] > R.useg[g]) { piece_t P; P.chunk = id; P.run = r; P.g = g; P.a = R.useg[g] - u0; P.b = R.useg[g + 1] - u0; pieces.push_back(std::move(P)); }
		S.chunk.push_back(std::move(buf)); S.chunk_len.push_back((size_t)uo); S.bytes += uo;
	}
	std::atomic<int> bad(0);
	parallel_for((int)std::min<size_t>((size_t)std::max(1, threads), pieces.size()), pieces.size(), [&](size_t a, size_t b, int) {
		for (size_t k = a; k < b; ++k) {
			piece_t &P = pieces[k]; const uint8_t *p = S.chunk[P.chunk].p; uint64_t o = P.a;
			while (o + 4 <= P.b) { uint32_t bs; memcpy(&bs, p + o, 4); if (o + 4 + (uint64_t)bs > P.b || bs < 32) { bad = 1; break; } P.loc.push_back((uint64_t)P.chunk << 40 | o); P.key.push_back(bam_sort_key(p + o + 4)); o += 4 + (uint64_t)bs; }
			if (o != P.b) bad = 1;
		}
	});
	if (bad) die("sort: a sorted run is damaged");
	size_t n = 0; for (const piece_t &P : pieces) n += P.loc.size();
	if (n >= 0xfffffff0u) die("sort: a stretch of the merge holds too many records (raise -m)");
	S.loc.resize(n); S.key.resize(n);
	{ std::vector<size_t> at(pieces.size() + 1, 0); for (size_t k = 0; k < pieces.size(); ++k) at[k + 1] = at[k] + pieces[k].loc.size();
	  const bool with_ord = !runs.empty() && runs[0].ord_fd >= 0;   /* rank mode: the records' input ordinals, from the runs' side files */
	  if (with_ord) S.ord.resize(n);
	  parallel_for((int)std::min<size_t>((size_t)std::max(1, threads), pieces.size()), pieces.size(), [&](size_t a, size_t b, int) {
		for (size_t k = a; k < b; ++k) {
			const piece_t &P = pieces[k];
			if (P.loc.empty()) continue;
			memcpy(&S.loc[at[k]], P.loc.data(), 8 * P.loc.size()); memcpy(&S.key[at[k]], P.key.data(), 8 * P.key.size());
			if (with_ord) {
				const run_t &R = runs[P.run];
				if (R.rcnt[P.g + 1] - R.rcnt[P.g] != P.loc.size()) { bad = 1; continue; }
				uint8_t *d = (uint8_t*)&S.ord[at[k]]; const size_t want = 8 * P.loc.size();
				for (size_t got = 0; got < want; ) { const ssize_t q = pread(R.ord_fd, d + got, want - got, (off_t)(8 * R.rcnt[P.g] + got)); if (q < 0 && errno == EINTR) continue; if (q <= 0) { bad = 1; break; } got += (size_t)q; }
			}
		} }); }
	if (bad) die("sort: a sorted run's ordinals are damaged");
}

/* order of a stretch's records: by key, equal keys by input ordinal when there are ordinals (rank mode: runs of several ranks hold records of
 * interleaved batches), else by position in the store (stable sort: earlier run first) */
static void stretch_perm(const rec_store_t &S, std::vector<uint32_t> &perm)
{
	if (S.ord.empty()) { gpu_perm(S, perm); return; }
	const size_t n = S.key.size();
	std::vector<uint32_t> p1(n), p2(n); std::vector<uint64_t> k1(n);
	if (ssg_sort_u64_perm(S.ord.data(), (int64_t)n, p1.data())) die(std::string("sort: ") + ssg_last_error());
	for (size_t i = 0; i < n; ++i) k1[i] = S.key[p1[i]];
	if (ssg_sort_u64_perm(k1.data(), (int64_t)n, p2.data())) die(std::string("sort: ") + ssg_last_error());
	perm.resize(n);
	for (size_t i = 0; i < n; ++i) perm[i] = p1[p2[i]];
}

/* g_lo .. g_hi: the ranges this call writes (all of them, or this rank's share in rank mode); seg_ret: where the header ended (rank mode's parts) */
static void merge_runs(std::vector<run_t> &runs, size_t G, const bam_hdr_t &h, int fd, int level, int threads, uint64_t budget, const char *bai_path, size_t g_lo = 0, size_t g_hi = (size_t)-1, uint64_t *hdr_end_ret = 0, const char *ent_path = 0)
{
	if (g_hi == (size_t)-1) g_hi = G;
	std::vector<size_t> cutg(1, g_lo);
	{	const uint64_t target = std::max<uint64_t>(budget / 3, 1); uint64_t acc = 0;
		for (size_t g = g_lo; g < g_hi; ++g) {
			uint64_t sz = 0; for (const run_t &R : runs) sz += R.useg[g + 1] - R.useg[g];
			if (acc && acc + sz > target) { cutg.push_back(g); acc = 0; }
			acc += sz;
		}
		cutg.push_back(g_hi);
	}
	const size_t ns = cutg.size() - 1;
	chan_t<std::unique_ptr<rec_store_t> > ch(1);
	std::thread loader([&]() {
		for (size_t k = 0; k < ns; ++k) { std::unique_ptr<rec_store_t> S(new rec_store_t()); load_stretch(runs, cutg[k], cutg[k + 1], threads, *S); ch.push(std::move(S)); }
		ch.close();
	});
	seg_out_t seg; double t_wait = 0, t_perm = 0, t_write = 0;
	if (ent_path) { seg.ent_fd = open(ent_path, O_WRONLY | O_CREAT | O_TRUNC, 0644); if (seg.ent_fd < 0) die(std::string("sort: cannot write ") + ent_path); }
	for (size_t k = 0; k < ns; ++k) {
		std::unique_ptr<rec_store_t> S;
		{ const double t0 = wall(); if (!ch.pop(S)) die("sort: the merge lost a stretch"); t_wait += wall() - t0; }
		seg.first = k == 0; seg.last = k + 1 == ns;
		std::vector<uint32_t> perm;
		{ const double t0 = wall(); stretch_perm(*S, perm); t_perm += wall() - t0; }
		{ const double t0 = wall(); write_sorted(*S, perm, h, fd, level, threads, bai_path, 0, 0, &seg); t_write += wall() - t0; }
	}
	loader.join();
	if (seg.ent_fd >= 0) close(seg.ent_fd);
	if (hdr_end_ret) *hdr_end_ret = seg.hdr_end;
	if (dbg()) fprintf(stderr, "[sambamba] sort: merge: %zu stretches of the genome; waited %.2f s for the loader (read + inflate + index of the runs), device sort of the keys %.2f s, gather + deflate + write %.2f s\n", ns, t_wait, t_perm, t_write);
}

/* rank mode, after a rank's part is written (by the merge of all ranks' runs, or from the blocks of the collective exchange): the markers the other ranks and
 * bin/speedseq-ranks wait for, and this rank's stretch placed in the joined file */
static bool place_part(const std::string &outp, const std::string &rdv, int rank, int world, uint64_t hdr_end)
{
		{ char t[64]; snprintf(t, sizeof(t), "%llu\n", (unsigned long long)hdr_end); if (!rk_file_put(outp + ".ssg_part", t, strlen(t))) die("sort: cannot write " + outp + ".ssg_part"); }
		/* the runs may go when every rank has read what it needed of them; the marker says how long this rank's part is and where its header blocks end */
		struct stat psb; if (stat(outp.c_str(), &psb) != 0) die("sort: cannot stat " + outp);
		{ char t[96]; snprintf(t, sizeof(t), "%llu %llu\n", (unsigned long long)psb.st_size, (unsigned long long)hdr_end); if (!rk_file_put(rdv + "/merged." + std::to_string(rank), t, strlen(t))) die("sort: cannot write into " + rdv); }
		for (int r = 0; r < world; ++r) if (!rk_file_wait(rdv + "/merged." + std::to_string(r))) die("sort: rank " + std::to_string(r) + " did not finish its merge");
		/* Every rank places its own stretch in the joined file (PREFIX.bam for a part named PREFIX.rank<r>.bam) at the offset the parts before it leave -- the
		 * stretches' lengths are only known now, so this is a copy, but N of them side by side instead of one by the launcher after the last rank has ended
		 * (the one term of the ranks' wall time that grew with the input and did not divide by N).  Part 0 goes with its header blocks, the others without; the
		 * last rank adds the end-of-file block; bin/speedseq-ranks finds joined.<r> of every rank and only indexes.  SSG_RANKS_JOIN=0 leaves the copy to it. */
		const std::string tail = ".rank" + std::to_string(rank) + ".bam";
		if (!(getenv("SSG_RANKS_JOIN") && !strcmp(getenv("SSG_RANKS_JOIN"), "0")) && outp.size() > tail.size() && outp.compare(outp.size() - tail.size(), tail.size(), tail) == 0) {
			const double tj = wall();
			uint64_t at = 0, my_from = 0, my_len = 0; bool ok = true;
			for (int r = 0; r < world && ok; ++r) {
				std::vector<uint8_t> b; unsigned long long sz = 0, he = 0;
				if (!rk_file_get(rdv + "/merged." + std::to_string(r), b)) { ok = false; break; }
				b.push_back(0);
				if (sscanf((const char*)b.data(), "%llu %llu", &sz, &he) != 2 || sz < 28 + he) { ok = false; break; }
				const uint64_t from = r ? he : 0, len = sz - 28 - from;
				if (r == rank) { my_from = from; my_len = len; break; }
				at += len;
			}
			const std::string joined = outp.substr(0, outp.size() - tail.size()) + ".bam";
			int jfd = ok ? open(joined.c_str(), O_WRONLY | O_CREAT, 0644) : -1, pfd = ok ? open(outp.c_str(), O_RDONLY) : -1;
			if (jfd >= 0 && pfd >= 0) {
				std::vector<uint8_t> buf;
				uint64_t done_b = 0;
				while (done_b < my_len && ok) {
					off64_t oi = (off64_t)(my_from + done_b), oo = (off64_t)(at + done_b);
					ssize_t k = copy_file_range(pfd, &oi, jfd, &oo, (size_t)std::min<uint64_t>(my_len - done_b, (uint64_t)1 << 30), 0);
					if (k <= 0) {   /* a file system that cannot: through a buffer */
						if (buf.empty()) buf.resize((size_t)8 << 20);
						k = pread(pfd, buf.data(), (size_t)std::min<uint64_t>(my_len - done_b, buf.size()), (off_t)(my_from + done_b));
						if (k <= 0) { ok = false; break; }
						for (ssize_t w = 0; w < k; ) { const ssize_t x = pwrite(jfd, buf.data() + w, (size_t)(k - w), (off_t)(at + done_b + (uint64_t)w)); if (x <= 0) { ok = false; break; } w += x; }
					}
					done_b += (uint64_t)k;
				}
				if (ok && rank == world - 1 && pwrite(jfd, BGZF_EOF, 28, (off_t)(at + my_len)) != 28) ok = false;
			} else ok = false;
			if (jfd >= 0 && close(jfd) != 0) ok = false;
			if (pfd >= 0) close(pfd);
			if (!ok) die("sort: cannot place this rank's stretch in " + joined);
			if (!rk_file_put(rdv + "/joined." + std::to_string(rank), "", 0)) die("sort: cannot write into " + rdv);
			if (dbg()) fprintf(stderr, "[sambamba] sort: rank %d placed its stretch (%.2f GB) at byte %llu of %s in %.2f s\n", rank, (double)my_len / 1e9, (unsigned long long)at, joined.c_str(), wall() - tj);
		}
	return true;
}

static int cmd_sort(int argc, char **argv)
{
	int threads = hw_threads(), level = -1; double mem_gb = 2; std::string tmpdir = ".", outp; const char *in = 0;
	for (int i = 0; i < argc; ++i) {
		const char *a = argv[i];
		if (!strcmp(a, "-t") && i + 1 < argc) threads = atoi(argv[++i]);
		else if (!strcmp(a, "-m") && i + 1 < argc) { const char *v = argv[++i]; char *e; mem_gb = strtod(v, &e); if (*e == 'M' || *e == 'm') mem_gb /= 1024; else if (*e == 'K' || *e == 'k') mem_gb /= 1048576; else if (!*e) mem_gb /= 1073741824.0; }
		else if (!strncmp(a, "--tmpdir=", 9)) tmpdir = a + 9;
		else if (!strcmp(a, "--tmpdir") && i + 1 < argc) tmpdir = argv[++i];
		else if (!strcmp(a, "-o") && i + 1 < argc) outp = argv[++i];
		else if (!strcmp(a, "-l") && i + 1 < argc) level = atoi(argv[++i]);
		else if (a[0] == '-' && a[1] && strcmp(a, "-")) die(std::string("sort: unsupported option ") + a);
		else in = a;
	}
	if (!in || outp.empty()) die("usage: sambamba sort [-t N] [-m XG] [--tmpdir=DIR] -o out.bam <in.bam>");
	if (threads < 1) threads = 1;
	const double t_start = wall();
	{ const char *e = getenv("SSG_BAM_LEVEL"); if (level < 0 && e && *e) level = atoi(e); }   /* deflate level of the sorted file when -l is not given (default: zlib's 6, as sambamba's) */
	bgzf_dev_level_set(level);
	/* compression is CPU work the reference's `-t` undersizes on a host with hundreds of cores next to an MI355X: the pool may use more (SSG_SORT_THREADS) */
	int pool = threads; { const char *e = getenv("SSG_SORT_THREADS"); if (e && atoi(e) > 0) pool = atoi(e); }
	pool = ssg_pool_threads(pool);
	const int fd = open_in(in);
	char first[8]; size_t n_first = 0;
	while (n_first < 8) { ssize_t r = read(fd, first + n_first, 8 - n_first); if (r < 0) { if (errno == EINTR) continue; die("sort: read error"); } if (r == 0) break; n_first += (size_t)r; }
	const bool fused = n_first == 8 && !memcmp(first, FU_MAGIC, 8);
	/* Rank mode (ranks.h): this sort holds the records of its rank's batches; all ranks' sorts exchange sorted runs through SSG_RDV and each
	 * writes the stretch of the genome it owns, as a BAM of its own that bin/speedseq-ranks joins to the others.  Only the main stream (frames)
	 * is exchanged: the side streams were brought to rank 0 by the samblasters already. */
	const int world = fused ? rk_world() : 1, rank = rk_rank();
	if (world > 1 && !rk_check("sambamba")) return 1;
	const std::string rdv = rk_dir(), rdata = rk_data_dir();
	/* the transport of the sorts' exchange (xchg.h: RCCL, sockets, or none = the files of rounds 4-5) comes up while the input streams in */
	xchg_t *X = 0; std::thread t_xchg;
	if (world > 1) t_xchg = std::thread([&]() { X = xchg_open(rank, world, rdv); });
	uint64_t budget = (uint64_t)(std::max(mem_gb, 0.25) * 0.6 * 1073741824.0);   /* record bytes per in-memory run; the rest is keys, locations, output blocks */
	{ const char *e = getenv("SSG_SORT_CHUNK_BYTES"); if (e && atoll(e) > 0) budget = (uint64_t)atoll(e); }   /* the tests force the spill-and-merge path */
	rec_store_t S; std::vector<std::string> spills; bam_hdr_t h;
	/* SSG_SORT_DEVICE_GATHER=1 (off by default): the records go to the device as they arrive and the final write gathers them there (dev_gather_t).  Only the single
	 * pipeline's final in-memory write at a compressing level, deflated and checksummed on the device; spilled runs, the merge and rank mode gather on the host. */
	dev_gather_t dg;
	{	const char *e = getenv("SSG_SORT_DEVICE_GATHER");
		if (e && *e && strcmp(e, "0")) {
			const char *const bdc = getenv("SSG_BGZF_DEVICE_CRC");
			const char *const why = world > 1 ? "rank mode" : level == 0 ? "level 0: nothing is deflated" : !bgzf_device_wanted() ? "the blocks are not deflated on the device"
			                      : bdc && !strcmp(bdc, "0") ? "SSG_BGZF_DEVICE_CRC=0: the host has no payload to checksum" : 0;
			uint64_t cap = budget; { const char *m = getenv("SSG_SORT_DEVICE_POOL_MB"); if (m && atoll(m) > 0) cap = (uint64_t)atoll(m) << 20; }   /* HBM for the records: the run's record budget */
			if (why) dev_gather_t::say_off(why); else dg.start(cap);
		}
	}
	/* the device is first needed when the last record has arrived: bring the runtime up now, next to the input, not then */
	std::thread warm([]() { const uint64_t k[2] = { 1, 0 }; uint32_t pm[2]; (void)ssg_sort_u64_perm(k, 2, pm); });
	struct joiner_t { std::thread &t; ~joiner_t() { if (t.joinable()) t.join(); } } warm_join = { warm };
	if (mkdir(tmpdir.c_str(), 0777) != 0 && errno != EEXIST) die("sort: cannot create " + tmpdir + ": " + strerror(errno));
	std::vector<run_t> runs; std::vector<uint64_t> range_lo;
	/* One run at a time; in the fused single-pipeline sort a run is written by a thread of its own while the input goes on into a second store (each of half the
	 * budget): until round 6 the input -- and with it samblaster and `bwa mem` -- stood still for as long as a run took to write. */
	rec_store_t S_bg; std::thread t_spill;
	auto spill_wait = [&]() { if (t_spill.joinable()) t_spill.join(); };
	auto spill_store = [&](rec_store_t &S) {
		std::vector<uint32_t> perm; gpu_perm(S, perm);
		if (runs.empty()) {   /* the ranges of the genome, fixed now: about 4 MB of a run each, so that one range of all runs is a small merge */
			size_t G = world > 1 ? 1024 : (size_t)std::min<uint64_t>(1024, std::max<uint64_t>(1, S.bytes >> 22));   /* rank mode: the same ranges on every rank */
			{ const char *e = getenv("SSG_SORT_RANGES"); if (e && atol(e) > 0) G = (size_t)atol(e); }
			make_ranges(h, G, range_lo);
		}
		const size_t G = range_lo.size(), n = perm.size();
		std::vector<size_t> at(G + 1, n);
		for (size_t g = 0; g < G; ++g) {   /* first record of the sorted order whose key reaches the range */
			size_t a = 0, b = n;
			while (a < b) { const size_t m = (a + b) >> 1; if (S.key[perm[m]] < range_lo[g]) a = m + 1; else b = m; }
			at[g] = a;
		}
		char nm[64]; snprintf(nm, sizeof(nm), "/ssg_sort_%d_%04zu.run", (int)getpid(), runs.size());
		if (world > 1) snprintf(nm, sizeof(nm), "/run.%d.%zu.run", rank, runs.size());
		run_t R; R.path = (world > 1 ? rdata : tmpdir) + nm;
		R.fd = open(R.path.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0644); if (R.fd < 0) die("sort: cannot write " + R.path);
		if (world > 1) {   /* equal keys keep their input order over all ranks: by ordinal within the run (the exchange sorts by it across runs) */
			std::vector<uint32_t> p1(n), p2(n); std::vector<uint64_t> k1(n);
			if (n && ssg_sort_u64_perm(S.ord.data(), (int64_t)n, p1.data())) die(std::string("sort: ") + ssg_last_error());
			for (size_t i = 0; i < n; ++i) k1[i] = S.key[p1[i]];
			if (n && ssg_sort_u64_perm(k1.data(), (int64_t)n, p2.data())) die(std::string("sort: ") + ssg_last_error());
			for (size_t i = 0; i < n; ++i) perm[i] = p1[p2[i]];
		}
		write_sorted(S, perm, h, R.fd, 1, pool, 0, &at, &R.seg, 0, &R.useg);
		if (world > 1) {   /* what the other ranks need of this run: segment offsets, record counts, ordinals in run order */
			std::vector<uint64_t> idx; idx.push_back((uint64_t)G);
			idx.insert(idx.end(), R.seg.begin(), R.seg.end()); idx.insert(idx.end(), R.useg.begin(), R.useg.end());
			for (size_t g = 0; g <= G; ++g) idx.push_back((uint64_t)at[g]);
			std::vector<uint64_t> od(n); for (size_t i = 0; i < n; ++i) od[i] = S.ord[perm[i]];
			if (!rk_file_put(R.path + ".ord", od.data(), 8 * n) || !rk_file_put(R.path + ".idx", idx.data(), 8 * idx.size())) die("sort: cannot write into " + rdata);
		}
		runs.push_back(R); spills.push_back(R.path); S.clear();
	};
	static const char *const dg_spill = "the records exceed the memory budget: sorted runs are spilled and merged";
	auto spill = [&]() { dg.stop(dg_spill); spill_wait(); spill_store(S); };
	const bool spill_bg = fused && world == 1 && !(getenv("SSG_SORT_SPILL_BG") && atoi(getenv("SSG_SORT_SPILL_BG")) == 0);
	auto spill_async = [&]() { dg.stop(dg_spill); spill_wait(); std::swap(S, S_bg); t_spill = std::thread([&]() { spill_store(S_bg); }); };
	struct spill_join_t { std::thread &t; ~spill_join_t() { if (t.joinable()) t.join(); } } spill_join = { t_spill };
	const uint64_t budget_in = spill_bg ? std::max<uint64_t>(budget / 2, 1) : budget;
	if (fused) {
		/* frames straight from samblaster (fused.h): a reader thread takes them off the pipe, this thread indexes the records (keys +
		 * locations) of each while the next arrives -- the sort's input work overlaps the alignment upstream */
		struct frame_t { fu_frame_t fh; fu_buf_t p; };
		chan_t<std::unique_ptr<frame_t> > ch(2); std::atomic<int> rd_fail(0);
		std::thread reader([&]() {
			for (;;) {
				std::unique_ptr<frame_t> F(new frame_t());
				if (!fu_read_frame(fd, F->fh, F->p)) { rd_fail = 1; fu_discard_rest(fd); break; }
				const bool end = F->fh.type == FU_END;
				ch.push(std::move(F));
				if (end) break;
			}
			ch.close();
		});
		std::unique_ptr<frame_t> F; bool ended = false; double t_wait = 0, t_index = 0; const char *bad = 0; uint64_t n_main = 0;   /* MAIN frames so far: frame k of rank r holds batch r + k * world */
		/* the page-locked staging blocks of the writer's producers (write_sorted: three producers, two slots and an output block each, 134 MB apiece) are made now, next
		 * to the input, and wait in the library's pool: page-locking 1.2 GB when the last record has arrived was a fifth of a second of the sort's tail.  Started with
		 * the first record frame -- by then `bwa mem' has its index on the device (the driver serialises page-locked allocations: see bwa_main.cpp). */
		std::thread prewarm; bool prewarmed = level == 0 || (getenv("SSG_SORT_PREWARM") && atoi(getenv("SSG_SORT_PREWARM")) == 0);
		struct prewarm_join_t { std::thread &t; ~prewarm_join_t() { if (t.joinable()) t.join(); } } prewarm_join = { prewarm };
		for (;;) {
			{ const double t0 = wall(); const bool got = ch.pop(F); t_wait += wall() - t0; if (!got) break; }
			if (F->fh.type == FU_END) { ended = true; break; }
			if (F->fh.type == FU_HEADER) { h.text.assign((const char*)F->p.p, (size_t)F->fh.len); hdr_from_text(h); change_so(h.text, "coordinate"); continue; }
			if (F->fh.type != FU_MAIN) { bad = "sort: unexpected frame in the fused stream"; break; }
			if (!F->fh.len) { ++n_main; continue; }
			if (!prewarmed) {
				prewarmed = true;
				prewarm = std::thread([]() {
					if (ssg_device_count() < 1 || !strcmp(ssg_backend(), "emu")) return;
					std::vector<void*> b;
					for (int k = 0; k < 9; ++k) b.push_back(ssg_host_alloc((size_t)2048 * (BGZF_MAX_PAYLOAD + 5) + 64));
					for (void *p : b) ssg_host_free(p);
				});
			}
			{ const double t0 = wall(); if (!S.add_chunk(std::move(F->p), (size_t)F->fh.len, world > 1 ? ((uint64_t)rank + n_main * (uint64_t)world) << 28 : ~(uint64_t)0)) { bad = "sort: malformed record frame"; break; } t_index += wall() - t0; }
			dg.push(S.chunk.back().p, S.chunk_len.back());
			++n_main;
			if (S.bytes >= budget_in || S.key.size() >= 0xfffffff0u) { if (spill_bg) spill_async(); else spill(); }
		}
		spill_wait();
		if (dbg()) fprintf(stderr, "[sambamba] sort: input thread waited %.2f s for frames, indexed records for %.2f s\n", t_wait, t_index);
		{ std::unique_ptr<frame_t> drop; while (ch.pop(drop)) {} }
		reader.join();                                           /* the rest of the stream was taken in (and its segments released) even after an error */
		if (bad) die(bad);
		if (rd_fail || !ended) die("sort: the fused stream ended early");
		if (h.names.empty() && h.text.empty()) change_so(h.text, "coordinate");
	} else {
		bgzf_in_t bi(fd, threads);
		bi.raw.assign((const uint8_t*)first, (const uint8_t*)first + n_first);
		if (!hdr_read(bi, h)) die("sort: not a BAM file");
		change_so(h.text, "coordinate");
		size_t CH = (size_t)std::min<uint64_t>((uint64_t)64 << 20, std::max<uint64_t>(budget / 4, 65536));   /* the budget is checked once per chunk */
		{ const char *e = getenv("SSG_SORT_IN_CHUNK_BYTES"); if (e && atoll(e) > 0) CH = (size_t)atoll(e); }   /* tests: a small file in several chunks, without a spill */
		fu_buf_t cur; size_t cap = CH, len = 0;
		if (!cur.heap(CH)) die("sort: out of memory");
		auto flush = [&]() { if (!len) return; if (!S.add_chunk(std::move(cur), len)) die("sort: malformed BAM record"); dg.push(S.chunk.back().p, S.chunk_len.back()); cap = CH; len = 0; if (!cur.heap(CH)) die("sort: out of memory"); if (S.bytes >= budget || S.key.size() >= 0xfffffff0u) spill(); };
		for (;;) {
			uint32_t bs;
			if (bi.get(&bs, 4) != 4) break;
			if (len + 4 + (size_t)bs > cap) {
				flush();
				if (4 + (size_t)bs > cap) { cap = 4 + (size_t)bs; if (!cur.heap(cap)) die("sort: out of memory"); }
			}
			memcpy(cur.p + len, &bs, 4);
			if (bi.get(cur.p + len + 4, bs) != bs) die("sort: truncated BAM");
			len += 4 + (size_t)bs;
		}
		flush();
	}
	ssg_recs_t *const recs = dg.finish();   /* (NULL unless every chunk is on the device) */
	const double t_in = wall();
	ssg_stamp("sambamba_sort", "input_done");
	bool bai_note = false;
	int ofd = open(outp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644); if (ofd < 0) die("sort: cannot write " + outp);
	if (world > 1) {
		t_xchg.join();
		if (X == (xchg_t*)-1) die("sort: the ranks' exchange transport failed to come up");
		if (X) {
			/* The collective form of the exchange (SURVEY.md 8e coupling 3): the records of this rank in (key, ordinal) order, cut at the stretches of the genome the ranks own (the
			 * same 1024 ranges as the file form, so the same records land on the same rank); sizes first, then one all-to-all of the blocks (ordinals + record bytes); the
			 * receiver orders what it got by (key, ordinal) on its device and writes its part.  Whether everybody can -- no rank has spilled, every rank's stretch fits its
			 * budget -- is itself agreed by an exchange; otherwise all ranks go on through the files. */
			const double t_x = wall();
			const size_t G = 1024; make_ranges(h, G, range_lo);
			std::vector<uint32_t> perm; stretch_perm(S, perm);
			const size_t n = perm.size();
			std::vector<size_t> cutp((size_t)world + 1, n);
			for (int d = 0; d < world; ++d) {
				const uint64_t lo_key = range_lo[G * (size_t)d / (size_t)world];
				size_t a = 0, b = n;
				while (a < b) { const size_t m = (a + b) >> 1; if (S.key[perm[m]] < lo_key) a = m + 1; else b = m; }
				cutp[(size_t)d] = a;
			}
			cutp[0] = 0;
			std::vector<uint64_t> cs((size_t)world * 3), cr((size_t)world * 3);
			for (int d = 0; d < world; ++d) {
				uint64_t bytes = 0;
				for (size_t i = cutp[(size_t)d]; i < cutp[(size_t)d + 1]; ++i) { uint32_t bs; memcpy(&bs, S.rec(perm[i]), 4); bytes += 4 + (uint64_t)bs; }
				cs[(size_t)d * 3] = cutp[(size_t)d + 1] - cutp[(size_t)d]; cs[(size_t)d * 3 + 1] = bytes; cs[(size_t)d * 3 + 2] = runs.empty() ? 1 : 0;
			}
			if (!X->alltoall_u64(cs.data(), cr.data(), 3)) die("sort: the ranks' exchange failed");
			uint64_t in_bytes = 0; bool all_ok = true;
			for (int q = 0; q < world; ++q) { in_bytes += cr[(size_t)q * 3 + 1]; if (!cr[(size_t)q * 3 + 2]) all_ok = false; }
			std::vector<uint64_t> f1((size_t)world, (all_ok && in_bytes <= budget * 2) ? 1 : 0), f2((size_t)world, 0);
			if (!X->alltoall_u64(f1.data(), f2.data(), 1)) die("sort: the ranks' exchange failed");
			for (int q = 0; q < world; ++q) if (!f2[(size_t)q]) all_ok = false;
			if (!all_ok) { if (rank == 0 && dbg()) fprintf(stderr, "[sambamba] sort: a rank's share does not fit its memory (or its input did not): the ranks exchange through files\n"); delete X; X = 0; }
			else {
				std::vector<std::vector<uint8_t> > sb((size_t)world), rb((size_t)world);
				std::vector<const void*> sp((size_t)world); std::vector<void*> rp((size_t)world); std::vector<uint64_t> sn((size_t)world), rn((size_t)world);
				parallel_for(std::min(pool, world), (size_t)world, [&](size_t a, size_t b, int) {
					for (size_t d = a; d < b; ++d) {
						const size_t nd = cutp[d + 1] - cutp[d];
						sb[d].resize(8 * nd + (size_t)cs[d * 3 + 1]);
						uint8_t *w = sb[d].data() + 8 * nd;
						for (size_t i = 0; i < nd; ++i) {
							const uint32_t id = perm[cutp[d] + i]; memcpy(sb[d].data() + 8 * i, &S.ord[id], 8);
							const uint8_t *r = S.rec(id); uint32_t bs; memcpy(&bs, r, 4); memcpy(w, r, 4 + (size_t)bs); w += 4 + (size_t)bs;
						}
					}
				});
				for (int q = 0; q < world; ++q) { rb[(size_t)q].resize(8 * (size_t)cr[(size_t)q * 3] + (size_t)cr[(size_t)q * 3 + 1]); sp[(size_t)q] = sb[(size_t)q].data(); rp[(size_t)q] = rb[(size_t)q].data(); sn[(size_t)q] = sb[(size_t)q].size(); rn[(size_t)q] = rb[(size_t)q].size(); }
				S.clear();
				if (!X->alltoallv(sp.data(), sn.data(), rp.data(), rn.data())) die("sort: the ranks' exchange failed");
				for (auto &v : sb) { std::vector<uint8_t>().swap(v); }
				rec_store_t R;
				for (int q = 0; q < world; ++q) {
					const size_t nq = (size_t)cr[(size_t)q * 3], len = (size_t)cr[(size_t)q * 3 + 1];
					if (!nq) continue;
					fu_buf_t c; if (!c.heap(len)) die("sort: out of memory");
					memcpy(c.p, rb[(size_t)q].data() + 8 * nq, len);
					std::vector<uint64_t> od(nq); memcpy(od.data(), rb[(size_t)q].data(), 8 * nq);
					std::vector<uint8_t>().swap(rb[(size_t)q]);
					if (!add_chunk_ords(R, std::move(c), len, od.data(), nq)) die("sort: a block of the ranks' exchange is not whole records");
				}
				std::vector<uint32_t> pr; stretch_perm(R, pr);
				seg_out_t seg; seg.first = true; seg.last = true;
				seg.ent_fd = open((outp + ".ssg_ent").c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644); if (seg.ent_fd < 0) die("sort: cannot write " + outp + ".ssg_ent");
				write_sorted(R, pr, h, ofd, level, pool, 0, 0, 0, &seg);
				close(seg.ent_fd); close(ofd);
				const uint64_t hdr_end = seg.hdr_end;
				if (dbg()) fprintf(stderr, "[sambamba] sort: rank %d of %d: %zu records of its own in, %zu records of its stretch out, exchanged over %s: %.2f s\n", rank, world, n, pr.size(), X->name(), wall() - t_x);
				delete X; X = 0;
				if (!place_part(outp, rdv, rank, world, hdr_end)) die("sort: cannot place this rank's stretch");
				return 0;
			}
		}
		/* every record of this rank goes into exchange runs (the last one now); then all ranks' runs are opened and this rank merges its share of the ranges */
		if (!S.key.empty() || runs.empty()) spill();
		const double t_x = wall();
		{ const uint64_t nr = runs.size(); if (!rk_file_put(rdv + "/sorted." + std::to_string(rank), &nr, 8)) die("sort: cannot write into " + rdv); }
		std::vector<run_t> all; size_t G = range_lo.size();
		for (int r = 0; r < world; ++r) {
			const std::string dn = rdv + "/sorted." + std::to_string(r); std::vector<uint8_t> b;
			if (!rk_file_wait(dn) || !rk_file_get(dn, b) || b.size() != 8) die("sort: rank " + std::to_string(r) + " did not deliver its runs");
			uint64_t nr; memcpy(&nr, b.data(), 8);
			for (uint64_t k = 0; k < nr; ++k) {
				run_t R; R.path = rdata + "/run." + std::to_string(r) + "." + std::to_string(k) + ".run";
				std::vector<uint8_t> ib;
				if (!rk_file_get(R.path + ".idx", ib) || ib.size() < 8) die("sort: cannot read " + R.path + ".idx");
				uint64_t g; memcpy(&g, ib.data(), 8);
				if (g != G || ib.size() != 8 * (1 + 3 * (g + 1))) die("sort: the ranks disagree about the ranges of the genome (different headers?)");
				const uint64_t *q = (const uint64_t*)(ib.data() + 8);
				R.seg.assign(q, q + g + 1); R.useg.assign(q + g + 1, q + 2 * (g + 1)); R.rcnt.assign(q + 2 * (g + 1), q + 3 * (g + 1));
				R.fd = open(R.path.c_str(), O_RDONLY); R.ord_fd = open((R.path + ".ord").c_str(), O_RDONLY);
				if (R.fd < 0 || R.ord_fd < 0) die("sort: cannot open " + R.path);
				all.push_back(R);
			}
		}
		const size_t g_lo = G * (size_t)rank / (size_t)world, g_hi = G * ((size_t)rank + 1) / (size_t)world;
		uint64_t hdr_end = 0;
		merge_runs(all, G, h, ofd, level, pool, budget, 0, g_lo, g_hi, &hdr_end, (outp + ".ssg_ent").c_str());
		close(ofd);
		if (!place_part(outp, rdv, rank, world, hdr_end)) die("sort: cannot place this rank's stretch");
		for (run_t &R : all) { close(R.fd); close(R.ord_fd); }
		for (run_t &R : runs) { close(R.fd); unlink(R.path.c_str()); unlink((R.path + ".ord").c_str()); unlink((R.path + ".idx").c_str()); }
		if (dbg()) fprintf(stderr, "[sambamba] sort: rank %d of %d: input %.2f s (from start), %zu run(s) of its own, ranges %zu .. %zu of %zu from %zu runs of all ranks: %.2f s\n", rank, world, t_in - t_start, runs.size(), g_lo, g_hi, G, all.size(), wall() - t_x);
		return 0;
	}
	if (spills.empty()) {
		std::vector<uint32_t> perm; gpu_perm(S, perm);
		const double t_perm = wall();
		const std::string bai = outp + ".bai";
		write_sorted(S, perm, h, ofd, level, pool, getenv("SSG_SORT_NO_BAI") ? 0 : bai.c_str(), 0, 0, 0, 0, recs);   /* (the store goes with the process: hipFree of gigabytes waits for the device) */
		bai_note = !getenv("SSG_SORT_NO_BAI");
		if (dbg()) fprintf(stderr, "[sambamba] sort: %zu records, %.2f GB: input %.2f s (from start), device sort of the keys %.2f s, gather + deflate (level %d, %d threads) + write %.2f s\n",
		                   S.key.size(), (double)S.bytes / 1e9, t_in - t_start, t_perm - t_in, level < 0 ? 6 : level, pool, wall() - t_perm);
	}
	else {
		if (!S.key.empty()) spill();
		const double t_m = wall();
		const std::string bai = outp + ".bai";
		merge_runs(runs, range_lo.size(), h, ofd, level, pool, budget, getenv("SSG_SORT_NO_BAI") ? 0 : bai.c_str());
		bai_note = !getenv("SSG_SORT_NO_BAI");
		if (dbg()) fprintf(stderr, "[sambamba] sort: input %.2f s (from start), %zu sorted runs merged in %zu ranges of the genome by %d threads: %.2f s\n", t_in - t_start, runs.size(), range_lo.size(), pool, wall() - t_m);
		for (run_t &R : runs) { close(R.fd); unlink(R.path.c_str()); }
	}
	close(ofd);
	if (bai_note) bai_note_write(outp);
	ssg_stamp("sambamba_sort", "written");
	ssg_worker_done(0);         /* (the record store's chunks are gigabytes of mapped frames: the script does not wait for them to be unmapped) */
	return ssg_fast_exit(0);
}

/* ---------------- index ---------------- */
/* `sambamba flagstat <in.bam>` (upstream sambamba has the command; the reference does not call it): the counts of samtools flagstat that
 * the soak's invariants need, in its line format, from the fixed fields only -- blocks inflated by the pool, one pass of a 100 GB file
 * in the time the reference's samtools needs for a few GB -- plus one line samtools does not print: whether the file is in coordinate
 * order (bam1_lt's key, unmapped reads last). */
static int cmd_flagstat(int argc, char **argv)
{
	const char *in = 0; int threads = hw_threads();
	for (int i = 0; i < argc; ++i) { if (!strcmp(argv[i], "-t") && i + 1 < argc) threads = atoi(argv[++i]); else if (argv[i][0] != '-') { if (!in) in = argv[i]; } }
	if (!in) die("usage: sambamba flagstat [-t N] <in.bam>");
	const int fd = open_in(in);
	bgzf_in_t bi(fd, threads); bam_hdr_t h;
	if (!hdr_read(bi, h)) die("flagstat: not a BAM file");
	uint64_t n = 0, sec = 0, sup = 0, dup = 0, mapped = 0, paired = 0, r1 = 0, r2 = 0, proper = 0, both = 0, single = 0, prim = 0, prim_dup = 0, descents = 0, prev = 0;
	uint8_t rec[32];
	for (;;) {
		uint32_t bs;
		if (bi.get(&bs, 4) != 4) break;
		if (bs < 32 || bi.get(rec, 32) != 32) die("flagstat: malformed BAM record");
		if (bi.skip(bs - 32) != bs - 32) die("flagstat: truncated BAM");
		bam_core_t c; memcpy(&c, rec, 32);
		const uint32_t f = c.flag_nc >> 16;
		++n;
		if (f & 0x100) ++sec; else if (f & 0x800) ++sup;
		if (f & 0x400) ++dup;
		if (!(f & 4)) ++mapped;
		if (!(f & 0x900)) { ++prim; if (f & 0x400) ++prim_dup; }
		if ((f & 1) && !(f & 0x900)) {
			++paired; if (f & 0x40) ++r1; if (f & 0x80) ++r2;
			if ((f & 2) && !(f & 4)) ++proper;
			if (!(f & 4) && !(f & 8)) ++both;
			if (!(f & 4) && (f & 8)) ++single;
		}
		const uint64_t key = (uint64_t)(uint32_t)c.tid << 32 | (uint32_t)((c.pos + 1) << 1) | ((f & 0x10) ? 1u : 0u);   /* tid -1 sorts last */
		if (n > 1 && key < prev) ++descents;
		prev = key;
	}
	close(fd);
	printf("%llu + 0 in total (QC-passed reads + QC-failed reads)\n%llu + 0 secondary\n%llu + 0 supplementary\n%llu + 0 duplicates\n%llu + 0 mapped\n%llu + 0 paired in sequencing\n%llu + 0 read1\n%llu + 0 read2\n"
	       "%llu + 0 properly paired\n%llu + 0 with itself and mate mapped\n%llu + 0 singletons\n%llu + 0 primary\n%llu + 0 primary duplicates\n%llu descents of the coordinate key (0 = sorted)\n",
	       (unsigned long long)n, (unsigned long long)sec, (unsigned long long)sup, (unsigned long long)dup, (unsigned long long)mapped, (unsigned long long)paired, (unsigned long long)r1, (unsigned long long)r2,
	       (unsigned long long)proper, (unsigned long long)both, (unsigned long long)single, (unsigned long long)prim, (unsigned long long)prim_dup, (unsigned long long)descents);
	return 0;
}

/* ---------------- merge and index on device-resident records (SSG_MERGE_DEVICE=1, SSG_INDEX_DEVICE=1) ----------------
 * The input is read as raw BGZF members, inflated into the record store (dev_batches_t, devread.h) and walked there (ssg_recs_scan): of every record 40 bytes come
 * back -- its location in the store, its sort key, the fields of its index entry -- and the payload stays in HBM.  `index' needs no more; `merge' declares the
 * merged order of what it has loaded (ssg_recs_order) and has the device gather, deflate and frame the output blocks (ssg_bgzf_compress_recs).
 * Both need a file whose blocks start at records (htslib's bgzf_flush_try, sambamba, this repository's writers); for any other they fall back on the host loops. */
static bool env_is_1(const char *name) { const char *e = getenv(name); return e && !strcmp(e, "1"); }
static const uint64_t LOC_OFF_MASK = ((uint64_t)1 << 40) - 1;

/* one load: the reader's next batch into the store, its records appended to loc / key / ent.  DEV_BATCH, DEV_END, or DEV_FAIL with `why' (the caller falls back, or ends); bad data ends the program as the host readers do */
static int dev_load(dev_batches_t &R, uint64_t &n_new, std::vector<uint64_t> &loc, std::vector<uint64_t> &key, std::vector<ssg_bam_ent_t> &ent, std::string &why)
{
	n_new = 0;
	const int got = R.next();
	if (got != DEV_BATCH) { why = R.why; return got; }
	const size_t nm = R.n(), have = loc.size(), cap = (size_t)(R.hint[nm] / 36) + 1;
	loc.resize(have + cap); key.resize(have + cap); ent.resize(have + cap);
	const int rc = ssg_recs_scan(R.recs, R.cid, R.hint.data(), (int64_t)nm, R.first, cap, &n_new, loc.data() + have, key.data() + have, ent.data() + have);
	/* (a stream the scan calls malformed goes to the host reader as well: a record that runs past the last of these members may be a truncated file, or one more block
	 * that does not start at a record -- the host reader tells them apart, and ends the program for the first) */
	if (rc) { n_new = 0; why = dev_stage_error(rc, R.name, "ssg_recs_scan: "); }
	loc.resize(have + n_new); key.resize(have + n_new); ent.resize(have + n_new);
	return rc ? DEV_FAIL : DEV_BATCH;
}

/* ---------------- view: selection (-F, -c, -o, -L, regions, -f bam with a BAM input) ----------------
 * What is read: without regions the whole file; with regions the chunks [u, v) of virtual offsets that the file's .bai gives for them (bai_reader_t, bamio.h:
 * hts_itr_query's candidates of every merged region, sorted and merged), each read from u until a record begins at or behind v.  The region test and the
 * filter decide on every record read.  The host path (the default, and the fall-back) inflates the members with zlib and runs view_region_keeps and
 * view_filter_keeps; SSG_VIEW_DEVICE=1 sends the same chunks through the record store and ssg_recs_select. */
typedef bai_reader_t::chunk_t view_chunk_t;
struct view_job_t {
	const char *in; int fd; bgzf_in_t *bi; bam_hdr_t h;   /* bi: the sequential reader, behind the header */
	std::vector<ssg_bam_region_t> reg; std::vector<ssg_bam_fop_t> prog; std::vector<view_chunk_t> chunks;
	bool count, with_hdr, bam_out; int level, threads, out_fd;
};
/* where the kept records of the host path go: SAM text, BAM blocks, or a count */
struct view_sink_t {
	view_job_t &J; std::string text; bgzf_out_t *bo; uint64_t n_kept;
	view_sink_t(view_job_t &j) : J(j), bo(0), n_kept(0)
	{
		if (J.count) return;
		if (J.bam_out) { bo = new bgzf_out_t(J.out_fd, J.level, J.threads); hdr_write(*bo, J.h); }
		else if (J.with_hdr) text = J.h.text;
	}
	void record(const uint8_t *rec, size_t len)
	{
		++n_kept;
		if (J.count) return;
		if (bo) { bo->record(rec, len); return; }
		if (!bam_record_to_sam(rec, hdr_name_of(J.h), text)) die("view: a record with a tag type this printer does not know");
		if (text.size() > ((size_t)1 << 20)) { io_write_all(J.out_fd, text.data(), text.size()); text.clear(); }
	}
	void finish()
	{
		if (J.count) text = std::to_string(n_kept) + "\n";
		if (bo) { bo->finish(); delete bo; bo = 0; }
		else io_write_all(J.out_fd, text.data(), text.size());
	}
};
static void view_host(view_job_t &J)
{
	view_sink_t sink(J);
	struct stat sb;
	if (J.chunks.size() == 1 && J.chunks[0].v == ~(uint64_t)0 && (fstat(J.fd, &sb) != 0 || !S_ISREG(sb.st_mode))) {   /* a pipe: the whole stream through the sequential reader */
		std::vector<uint8_t> rec;
		for (;;) {
			uint32_t bs;
			if (J.bi->get(&bs, 4) != 4) break;
			if (bs < 32) die("view: malformed BAM record");
			rec.resize(4 + (size_t)bs); memcpy(rec.data(), &bs, 4);
			if (J.bi->get(rec.data() + 4, bs) != bs) die("view: truncated BAM");
			if (32 + (size_t)rec[12] + 4 * ((size_t)rec[16] | (size_t)rec[17] << 8) > bs) die("view: malformed BAM record");
			if (view_region_keeps(J.reg, rec.data()) && view_filter_keeps(J.prog, rec.data())) sink.record(rec.data(), rec.size());
		}
		sink.finish();
		return;
	}
	raw_members_t rd; std::vector<uint8_t> stream; std::vector<uint64_t> mstart, maddr, out_off;
	for (const view_chunk_t &c : J.chunks) {
		const bool whole = c.v == ~(uint64_t)0;
		rd.start(J.fd, J.in, c.u >> 16);
		stream.clear(); mstart.clear(); maddr.clear();
		uint64_t pos = c.u & 0xffff; size_t m = 0; bool done = false;
		while (!done && rd.next(whole ? (uint64_t)64 << 20 : (uint64_t)2 << 20, whole ? 1024 : 32)) {
			const size_t nm = rd.n(), base = stream.size();
			out_off.assign(nm + 1, 0);
			for (size_t k = 0; k < nm; ++k) { uint32_t isz; memcpy(&isz, rd.buf.data() + rd.moff[k + 1] - 4, 4); if (isz > 65536) die(std::string("view: a BGZF block that claims more than 64 KB in ") + J.in); out_off[k + 1] = out_off[k] + isz; }
			stream.resize(base + (size_t)out_off[nm]);
			std::vector<int> bad(nm, 0);
			parallel_for(J.threads, nm, [&](size_t a, size_t b, int) {
				for (size_t k = a; k < b; ++k) {
					const uint8_t *mb = rd.buf.data() + rd.moff[k]; const size_t len = (size_t)(rd.moff[k + 1] - rd.moff[k]), xlen = mb[10] | (size_t)mb[11] << 8;
					z_stream z; memset(&z, 0, sizeof(z));
					if (len < 12 + xlen + 8 || inflateInit2(&z, -15) != Z_OK) { bad[k] = 1; continue; }
					z.next_in = (Bytef*)(mb + 12 + xlen); z.avail_in = (uInt)(len - 12 - xlen - 8);
					z.next_out = stream.data() + base + out_off[k]; z.avail_out = (uInt)(out_off[k + 1] - out_off[k]);
					const int rc = inflate(&z, Z_FINISH);
					if (rc != Z_STREAM_END || z.avail_out != 0) bad[k] = 1;
					inflateEnd(&z);
				}
			});
			for (size_t k = 0; k < nm; ++k) {
				if (bad[k]) die(std::string("view: inflate failed: BGZF member at file offset ") + std::to_string(rd.addr + rd.moff[k]) + " of " + J.in);
				mstart.push_back(base + out_off[k]); maddr.push_back(rd.addr + rd.moff[k]);
			}
			if (pos > stream.size()) die(std::string("view: the index of ") + J.in + " points behind a block's end");
			while (pos + 4 <= stream.size()) {
				uint32_t bs; memcpy(&bs, stream.data() + pos, 4);
				if (bs < 32) die("view: malformed BAM record");
				if (pos + 4 + (uint64_t)bs > stream.size()) break;
				while (m + 1 < mstart.size() && mstart[m + 1] <= pos) ++m;                  /* the member that holds the record's first byte */
				if ((maddr[m] << 16 | (pos - mstart[m])) >= c.v) { done = true; break; }
				const uint8_t *rec = stream.data() + pos;
				if (32 + (size_t)rec[12] + 4 * ((size_t)rec[16] | (size_t)rec[17] << 8) > bs) die("view: malformed BAM record");   /* (its end is read from its CIGAR) */
				if (view_region_keeps(J.reg, rec) && view_filter_keeps(J.prog, rec)) sink.record(rec, 4 + (size_t)bs);
				pos += 4 + (uint64_t)bs;
			}
			/* what is consumed leaves the buffer */
			while (m + 1 < mstart.size() && mstart[m + 1] <= pos) ++m;
			const uint64_t drop = std::min<uint64_t>(mstart[m], pos);
			if (drop) {
				stream.erase(stream.begin(), stream.begin() + (ptrdiff_t)drop); pos -= drop;
				mstart.erase(mstart.begin(), mstart.begin() + (ptrdiff_t)m); maddr.erase(maddr.begin(), maddr.begin() + (ptrdiff_t)m); m = 0;
				for (uint64_t &s : mstart) s -= drop;
			}
		}
		if (!done && pos != stream.size()) die("view: truncated BAM");
	}
	sink.finish();
}

/* the BGZF members of a file, counted from their headers (the last line of the device path's log) */
static uint64_t view_count_members(int fd)
{
	uint64_t n = 0, at = 0; uint8_t hd[18];
	while (pread(fd, hd, 18, (off_t)at) == 18 && hd[0] == 0x1f && hd[1] == 0x8b && hd[12] == 'B' && hd[13] == 'C') { at += (uint64_t)(hd[16] | (size_t)hd[17] << 8) + 1; ++n; }
	return n;
}

/* The device path: every chunk's whole members from u >> 16 through the member that holds v go into the store in batches of at most 4096 members or 256 MB
 * (ssg_recs_release after each); the stream of a batch begins at `first' (u & 0xffff in a chunk's first batch) and ends, in the chunk's last member, at v's
 * offset: both are record starts by the index's construction.  ssg_recs_select decides and compacts.  -c: the counting form, two integers a batch.  SAM text:
 * the kept records declared as the stream (ssg_recs_order), gathered (ssg_recs_gather) and printed by bam_record_to_sam.  BAM: the header's blocks from the
 * host, the kept records' blocks cut by bgzf_out_t::record's rule (a batch ends its last block) and gathered, deflated and framed on the device
 * (ssg_bgzf_compress_recs_level, as the device merge writes them), the end-of-file marker last.  false with `why' while nothing is written: the host path
 * takes over; once output has begun a failure ends the command. */
static bool view_device(view_job_t &J, std::string &why)
{
	if (J.bam_out && !J.count && J.level == 0) { why = "-l 0: stored blocks are the host's"; return false; }
	if (!dev_read_ready(J.fd, why)) return false;
	recs_holder_t S;
	const char *const pool = getenv("SSG_VIEW_POOL");   /* bytes the record store may hold (tests: a batch beyond it is a store failure) */
	if (ssg_set_device(0) || ssg_recs_create(pool && *pool ? strtoull(pool, 0, 10) : ~(uint64_t)0 >> 1, &S.r)) { why = ssg_last_error(); return false; }
	dev_prof_begin();
	const bool bam = J.bam_out && !J.count;
	if (bam) bgzf_dev_level_set(J.level);
	const long BATCH = 1024;   /* blocks per device call */
	const uint64_t out_cap = bam ? ssg_bgzf_bound((uint64_t)BATCH * BGZF_MAX_PAYLOAD, BATCH) : 0;
	host_pinned_t O;
	if (bam && !O.grow(out_cap)) { why = "no page-locked memory for the output blocks"; return false; }
	dev_batches_t R; R.init("view", S.r, J.fd, J.in, (uint64_t)256 << 20, 4096); R.chunks = J.chunks;
	uint64_t n_scanned = 0, n_kept = 0, n_members = 0, n_blocks = 0; int n_batches = 0; bool begun = false;
	std::vector<uint64_t> loc, key, cum, cut, boff((size_t)BATCH + 1); std::vector<ssg_bam_ent_t> ent; std::vector<uint8_t> buf;
	std::string text; if (J.with_hdr && !J.count && !bam) text = J.h.text;
	const double t0 = wall();
	auto fail = [&](const std::string &m) -> bool { if (begun) die("view: " + m + " after output had begun (SSG_VIEW_DEVICE=0 reads the file on the host)"); why = m; return false; };
	auto begin_bam = [&]() { if (!begun) { bgzf_out_t o(J.out_fd, J.level, J.threads); hdr_write(o, J.h); o.drain(true); begun = true; } };
	for (int got; (got = R.next()) != DEV_END; ) {
		if (got == DEV_FAIL) return fail(R.why);
		const size_t nm = R.n();
		uint64_t n_rec = 0, n_sel = 0;
		const uint64_t cap = J.count ? 0 : R.hint[nm] / 36 + 1;
		if (!J.count) { loc.resize((size_t)cap); key.resize((size_t)cap); ent.resize((size_t)cap); }
		const int rc = ssg_recs_select(S.r, R.cid, R.hint.data(), (int64_t)nm, R.first, J.reg.empty() ? 0 : J.reg.data(), (int64_t)J.reg.size(), J.prog.empty() ? 0 : J.prog.data(), (int)J.prog.size(), cap, &n_rec, &n_sel,
		                               J.count ? 0 : loc.data(), J.count ? 0 : key.data(), J.count ? 0 : ent.data());
		if (rc) return fail(dev_stage_error(rc, J.in, "ssg_recs_select: "));
		if (!J.count && n_sel) {
			cum.resize((size_t)n_sel + 1); cum[0] = 0;
			for (uint64_t i = 0; i < n_sel; ++i) cum[(size_t)i + 1] = cum[(size_t)i] + ent[(size_t)i].len;
			if (ssg_recs_order(S.r, loc.data(), cum.data(), (int64_t)n_sel)) return fail(ssg_last_error());
			if (bam) {
				bgzf_cut_blocks(cum.data(), (size_t)n_sel, cut);   /* (a batch ends its last block) */
				const size_t nb = cut.size() - 1;
				for (size_t b0 = 0; b0 < nb; b0 += (size_t)BATCH) {
					const long k = (long)std::min<size_t>((size_t)BATCH, nb - b0);
					if (dev_bgzf_compress_recs(S.r, cut.data() + b0, k, O.p, out_cap, boff.data(), 0)) return fail(ssg_last_error());
					begin_bam();
					io_write_all(J.out_fd, O.p, (size_t)boff[(size_t)k]);
				}
				n_blocks += nb;
			} else {
				buf.resize((size_t)cum[(size_t)n_sel]);
				if (ssg_recs_gather(S.r, 0, cum[(size_t)n_sel], buf.data())) return fail(ssg_last_error());
				for (uint64_t i = 0; i < n_sel; ++i) {
					if (!bam_record_to_sam(buf.data() + cum[(size_t)i], hdr_name_of(J.h), text)) die("view: a record with a tag type this printer does not know");
					if (text.size() > ((size_t)1 << 20)) { io_write_all(J.out_fd, text.data(), text.size()); text.clear(); begun = true; }
				}
			}
			if (ssg_recs_reopen(S.r)) return fail(ssg_last_error());
		}
		if (ssg_recs_release(S.r, R.cid)) return fail(ssg_last_error());
		n_scanned += n_rec; n_kept += n_sel; n_members += nm; ++n_batches;
	}
	if (J.count) text = std::to_string(n_kept) + "\n";
	if (bam) { begin_bam(); io_write_all(J.out_fd, BGZF_EOF, 28); }
	else io_write_all(J.out_fd, text.data(), text.size());
	dev_prof_report("sambamba", "view");
	if (dbg()) fprintf(stderr, "[sambamba] view: on the device: %llu of %llu members read, %llu records scanned, %llu kept, %d batches%s, %.2f s\n", (unsigned long long)n_members, (unsigned long long)view_count_members(J.fd),
	                   (unsigned long long)n_scanned, (unsigned long long)n_kept, n_batches, bam ? (", " + std::to_string(n_blocks) + " blocks" + bgzf_dev_level_note()).c_str() : "", wall() - t0);
	return true;
}

static void view_select(view_job_t &J, bool with_regions);
static void view_select_run(const char *in, int fd, bgzf_in_t *bi, bam_hdr_t &h, uint64_t v0, std::vector<ssg_bam_region_t> &reg, bool with_regions, const std::vector<ssg_bam_fop_t> &prog, bool count, bool with_hdr, bool bam_out, int level, int threads, int out_fd)
{
	view_job_t J; J.in = in; J.fd = fd; J.bi = bi; J.h = h; J.reg = reg; J.prog = prog; J.count = count; J.with_hdr = with_hdr; J.bam_out = bam_out; J.level = level; J.threads = threads; J.out_fd = out_fd;
	view_chunk_t all; all.u = v0; all.v = ~(uint64_t)0; J.chunks.assign(1, all);
	view_select(J, with_regions);
}
static void view_select(view_job_t &J, bool with_regions)
{
	if (with_regions) bai_chunks_for("view", J.in, J.fd, J.h.names.size(), J.reg, J.chunks);   /* the index says what to read */
	if (env_is_1("SSG_VIEW_DEVICE")) {
		std::string why;
		if (view_device(J, why)) return;
		if (dbg()) fprintf(stderr, "[sambamba] view: device view off (%s): the file is read on the host\n", why.c_str());
	}
	view_host(J);
}

/* `sambamba index' from the device: true when the .bai is written; false with `why' -- nothing was written, the host loop takes over */
static bool index_device(const char *in, int fd, int n_ref, uint64_t v0, std::string &why)
{
	if (!dev_read_ready(fd, why)) return false;
	recs_holder_t S;
	if (ssg_set_device(0) || ssg_recs_create(~(uint64_t)0 >> 1, &S.r)) { why = ssg_last_error(); return false; }
	dev_prof_begin();
	dev_batches_t R; R.init("index", S.r, fd, in, (uint64_t)256 << 20, 4096); R.whole_file(v0);   /* a batch: the 4096 members of one device call of the inflate, at most 256 MB of records */
	const raw_members_t &rd = R.rd; const std::vector<uint64_t> &out_off = R.hint;
	bai_t idx(n_ref, v0);
	uint64_t n_total = 0; bool have = false; ssg_bam_ent_t p; memset(&p, 0, sizeof(p));
	std::vector<uint64_t> loc, key; std::vector<ssg_bam_ent_t> ent;
	const double t0 = wall(); double t_dev = 0;
	for (;;) {
		uint64_t n = 0; loc.clear(); key.clear(); ent.clear();
		const double t1 = wall();
		const int got = dev_load(R, n, loc, key, ent, why);
		if (got == DEV_FAIL) return false;
		if (got == DEV_END) break;
		t_dev += wall() - t1;
		size_t m = 0;
		for (uint64_t i = 0; i < n; ++i) {   /* the record's virtual offset: the member that holds its first byte (one without bytes holds none) */
			const uint64_t o = loc[i] & LOC_OFF_MASK;
			while (out_off[m + 1] <= o) ++m;
			const uint64_t v = (rd.addr + rd.moff[m]) << 16 | (o - out_off[m]);
			if (have && idx.push(p.tid, p.pos, p.end, v, !(p.flag & 4)) < 0) die("index: the file is not coordinate-sorted");
			p = ent[i]; have = true;
		}
		n_total += n;
		if (ssg_recs_release(S.r, R.cid)) { why = ssg_last_error(); return false; }
	}
	const uint64_t eof_v = rd.end_addr() << 16;
	if (have && idx.push(p.tid, p.pos, p.end, eof_v, !(p.flag & 4)) < 0) die("index: the file is not coordinate-sorted");
	idx.finish(eof_v);
	idx.save((std::string(in) + ".bai").c_str());
	dev_prof_report("sambamba", "index");
	if (dbg()) fprintf(stderr, "[sambamba] index: %llu records found on the device in %.2f s (inflate into the store + scan %.2f s)\n", (unsigned long long)n_total, wall() - t0, t_dev);
	return true;
}

/* one input of the device merge: its reader, and what is loaded of it and not yet written, in file order */
struct dm_src_t {
	dev_batches_t R; bool ended; uint64_t n_seen, last_key, pend_bytes;
	std::vector<uint64_t> loc, key; std::vector<ssg_bam_ent_t> ent;
	std::deque<std::pair<uint32_t, uint64_t> > chunks;   /* chunk id, its records not yet written */
	dm_src_t() : ended(false), n_seen(0), last_key(0), pend_bytes(0) {}
};

/* `sambamba merge' on the device.  true: the file, its .bai and the note are written.  false with `why': nothing was written, the host merge takes over.
 * A failure after output began ends the program (the partial file is removed). */
static bool merge_device(const std::vector<const char*> &files, std::vector<merge_src_t> &src, const bam_hdr_t &h, int level, int threads, std::string &why)
{
	const size_t F = src.size();
	if (level == 0) { why = "-l 0: the device writes no stored blocks"; return false; }
	for (size_t f = 0; f < F; ++f) if (!dev_read_ready(src[f].fd, why)) return false;
	recs_holder_t S;
	if (ssg_set_device(0)) { why = ssg_last_error(); return false; }
	/* HBM: a quarter of what is free for the records (the rest: what is loaded and not yet written of the inputs that are ahead, the members on their way in, the
	 * gathered and deflated blocks on their way out), split over the inputs, at most 1 GB each (one load takes at most the 4096 members of one device call of the inflate, 256 MB); SSG_MERGE_WINDOW and SSG_MERGE_POOL (bytes) override */
	uint64_t hbm_free = 0, hbm_total = 0;
	if (ssg_device_memory(&hbm_free, &hbm_total)) { why = ssg_last_error(); return false; }
	uint64_t window = std::min<uint64_t>((uint64_t)1 << 30, std::max<uint64_t>(hbm_free / 4 / F, (uint64_t)1 << 20)), pool = hbm_free / 2;
	{ const char *e = getenv("SSG_MERGE_WINDOW"); if (e && atoll(e) > 0) window = (uint64_t)atoll(e); }
	{ const char *e = getenv("SSG_MERGE_POOL"); if (e && atoll(e) > 0) pool = (uint64_t)atoll(e); }
	if (ssg_recs_create(pool, &S.r)) { why = ssg_last_error(); return false; }
	dev_prof_begin();
	std::vector<dm_src_t> in(F);
	for (size_t f = 0; f < F; ++f) { in[f].R.init("merge", S.r, src[f].fd, files[f + 1], window, 4096); in[f].R.whole_file(src[f].in->tell()); }
	int ofd = -1; uint64_t coff = 0;
	auto fail = [&](const std::string &m) {   /* after output began */
		if (ofd >= 0) { close(ofd); unlink(files[0]); }
		die("merge: " + m + "; the partial output was removed -- SSG_MERGE_DEVICE=0 merges on the host");
	};
	/* an input that has less than half a window loaded takes its next members (a round loads every input at the start; an input that is ahead of the others waits) */
	auto load = [&](bool &ok) {
		ok = true;
		for (size_t f = 0; f < F && ok; ++f) {
			dm_src_t &s = in[f];
			while (!s.ended && (s.key.empty() || s.pend_bytes < window / 2)) {
				uint64_t n = 0; const size_t have = s.key.size();
				const int got = dev_load(s.R, n, s.loc, s.key, s.ent, why);
				if (got == DEV_END) { s.ended = true; break; }
				if (got == DEV_FAIL) { ok = false; break; }
				const uint32_t cid = s.R.cid;
				for (size_t i = have; i < have + n; ++i) {
					if (s.n_seen && s.key[i] < s.last_key) { const std::string m = std::string(files[f + 1]) + " is not coordinate-sorted: its record " + std::to_string(s.n_seen) + " (counted from 0) descends"; if (ofd >= 0) fail(m); die("merge: " + m); }
					s.last_key = s.key[i]; ++s.n_seen; s.pend_bytes += s.ent[i].len;
				}
				if (n) s.chunks.push_back(std::make_pair(cid, n));
				else if (ssg_recs_release(S.r, cid)) { ok = false; why = ssg_last_error(); break; }
				if (s.R.rd.at_end) s.ended = true;
				if (s.key.size() > have) break;   /* (one load a round for an input that got records) */
			}
		}
	};
	bool ok = true;
	load(ok);
	if (!ok) return false;
	bool any = false; for (const dm_src_t &s : in) any = any || !s.key.empty();
	/* from here on there is output */
	ofd = open(files[0], O_WRONLY | O_CREAT | O_TRUNC, 0644); if (ofd < 0) die(std::string("merge: cannot write ") + files[0]);
	{ bgzf_out_t out(ofd, level, threads); hdr_write(out, h); out.drain(true); }
	{ const off_t o = lseek(ofd, 0, SEEK_CUR); if (o < 0) fail("the output cannot be sought"); coff = (uint64_t)o; }
	bai_t idx((int)h.names.size(), (any ? coff : coff + 28) << 16);
	bool have_p = false; ssg_bam_ent_t p; memset(&p, 0, sizeof(p));
	const long BATCH = 1024;   /* blocks per device call: 64 MB of records */
	const uint64_t out_cap = ssg_bgzf_bound((uint64_t)BATCH * BGZF_MAX_PAYLOAD, BATCH);
	host_pinned_t O;
	if (!O.grow(out_cap)) fail("no page-locked memory for the output blocks");
	std::vector<uint64_t> keys, sloc, cum, cut, boff((size_t)BATCH + 1); std::vector<uint32_t> perm, from; std::vector<ssg_bam_ent_t> sent; std::vector<size_t> take(F), base(F + 1);
	uint64_t n_written = 0, n_rounds = 0, n_blocks = 0; const double t0 = wall(); double t_load = 0, t_sort = 0, t_write = 0;
	for (;;) {
		/* what may be written: everything below the smallest last key of the inputs that have not ended -- what they have not loaded yet sorts behind it */
		bool all_ended = true; uint64_t Kb = 0; size_t fb = 0;
		for (size_t f = 0; f < F; ++f) if (!in[f].ended) { const uint64_t K = in[f].key.back(); if (all_ended || K < Kb) { Kb = K; fb = f; } all_ended = false; }
		uint64_t E = 0;
		for (size_t f = 0; f < F; ++f) {
			const std::vector<uint64_t> &k = in[f].key;
			take[f] = all_ended ? k.size() : (size_t)((f <= fb ? std::upper_bound(k.begin(), k.end(), Kb) : std::lower_bound(k.begin(), k.end(), Kb)) - k.begin());
			base[f] = (size_t)E; E += take[f];
		}
		base[F] = (size_t)E;
		if (E >= ((uint64_t)1 << 32)) fail("more than 2^32 records in one round: a smaller SSG_MERGE_WINDOW is needed");
		if (E) {
			const double t1 = wall();
			/* the merged order (key, input, position in the input): the inputs' keys one after the other, sorted by a stable sort */
			keys.resize((size_t)E); perm.resize((size_t)E);
			for (size_t f = 0; f < F; ++f) std::copy(in[f].key.begin(), in[f].key.begin() + (ptrdiff_t)take[f], keys.begin() + (ptrdiff_t)base[f]);
			if (ssg_sort_u64_perm(keys.data(), (int64_t)E, perm.data())) fail(ssg_last_error());
			sloc.resize((size_t)E); sent.resize((size_t)E); cum.resize((size_t)E + 1); cum[0] = 0;
			for (uint64_t j = 0; j < E; ++j) {
				const size_t g = perm[(size_t)j], f = (size_t)(std::upper_bound(base.begin(), base.end(), g) - base.begin()) - 1, i = g - base[f];
				sloc[(size_t)j] = in[f].loc[i]; sent[(size_t)j] = in[f].ent[i]; cum[(size_t)j + 1] = cum[(size_t)j] + in[f].ent[i].len;
			}
			bgzf_cut_blocks(cum.data(), (size_t)E, cut);   /* (a round ends its last block) */
			t_sort += wall() - t1;
			const double t2 = wall();
			if (ssg_recs_order(S.r, sloc.data(), cum.data(), (int64_t)E)) fail(ssg_last_error());
			const size_t nb = cut.size() - 1; uint64_t j = 0;
			for (size_t b0 = 0; b0 < nb; b0 += (size_t)BATCH) {
				const long k = (long)std::min<size_t>((size_t)BATCH, nb - b0);
				if (dev_bgzf_compress_recs(S.r, cut.data() + b0, k, O.p, out_cap, boff.data(), 0)) fail(ssg_last_error());
				io_write_all(ofd, O.p, (size_t)boff[(size_t)k]);
				/* the index entries of the records that begin in these blocks: an entry closes at the virtual offset of the record behind it */
				size_t b = b0;
				for (; j < E && cum[(size_t)j] < cut[b0 + (size_t)k]; ++j) {
					while (cut[b + 1] <= cum[(size_t)j]) ++b;
					const uint64_t v = (coff + boff[b - b0]) << 16 | (cum[(size_t)j] - cut[b]);
					if (have_p && idx.push(p.tid, p.pos, p.end, v, !(p.flag & 4)) < 0) fail("the merged records are not in coordinate order");
					p = sent[(size_t)j]; have_p = true;
				}
				coff += boff[(size_t)k];
			}
			n_blocks += nb;
			if (ssg_recs_reopen(S.r)) fail(ssg_last_error());
			/* what is written leaves the host lists, and a chunk all of whose records are written leaves the device */
			for (size_t f = 0; f < F; ++f) {
				dm_src_t &s = in[f]; uint64_t t = take[f];
				for (size_t i = 0; i < take[f]; ++i) s.pend_bytes -= s.ent[i].len;
				s.loc.erase(s.loc.begin(), s.loc.begin() + (ptrdiff_t)take[f]); s.key.erase(s.key.begin(), s.key.begin() + (ptrdiff_t)take[f]); s.ent.erase(s.ent.begin(), s.ent.begin() + (ptrdiff_t)take[f]);
				while (t) {
					std::pair<uint32_t, uint64_t> &c = s.chunks.front(); const uint64_t d = std::min(t, c.second);
					c.second -= d; t -= d;
					if (!c.second) { if (ssg_recs_release(S.r, c.first)) fail(ssg_last_error()); s.chunks.pop_front(); }
				}
			}
			n_written += E; ++n_rounds;
			t_write += wall() - t2;
		}
		if (all_ended) break;
		const double t3 = wall();
		load(ok);
		if (!ok) fail(why);
		t_load += wall() - t3;
	}
	io_write_all(ofd, BGZF_EOF, 28);
	const uint64_t eof_v = (coff + 28) << 16;
	if (have_p && idx.push(p.tid, p.pos, p.end, eof_v, !(p.flag & 4)) < 0) fail("the merged records are not in coordinate order");
	idx.finish(eof_v);
	if (close(ofd) != 0) { ofd = -1; fail(std::string("cannot write ") + files[0]); }
	idx.save((std::string(files[0]) + ".bai").c_str());
	bai_note_write(files[0]);
	dev_prof_report("sambamba", "merge");
	if (dbg()) fprintf(stderr, "[sambamba] merge: %llu records of %zu inputs merged on the device in %llu round(s) of at most %llu bytes an input: %llu blocks, %.2f s (after the first load: inflate + scan %.2f s, order %.2f s, gather + deflate + write %.2f s)%s\n",
	                   (unsigned long long)n_written, F, (unsigned long long)n_rounds, (unsigned long long)window, (unsigned long long)n_blocks, wall() - t0, t_load, t_sort, t_write, bgzf_dev_level_note().c_str());
	return true;
}

static int cmd_index(int argc, char **argv)
{
	const char *in = 0; int threads = hw_threads();
	for (int i = 0; i < argc; ++i) { if (!strcmp(argv[i], "-t") && i + 1 < argc) threads = atoi(argv[++i]); else if (argv[i][0] != '-') { if (!in) in = argv[i]; } }
	if (!in) die("usage: sambamba index <in.bam>");
	if (rk_world() > 1) {   /* rank mode: a rank's stretch of the sorted file is not what gets indexed -- bin/speedseq-ranks indexes the joined file */
		struct stat sb;
		if (stat((std::string(in) + ".ssg_part").c_str(), &sb) == 0) { if (dbg()) fprintf(stderr, "[sambamba] index: %s is one rank's part of a sorted file: left to the join\n", in); return 0; }
	}
	{	/* the sort of this repository left the index of exactly this file next to it: nothing to do (the note goes, the pair stays) */
		const std::string note_p = std::string(in) + ".bai.ssg";
		FILE *f = fopen(note_p.c_str(), "r");
		if (f) {
			char have[128] = ""; if (!fgets(have, sizeof(have), f)) have[0] = 0;
			fclose(f); unlink(note_p.c_str());
			std::string now;
			if (bai_note_make(in, now) && now == have) { if (dbg()) fprintf(stderr, "[sambamba] index: %s.bai written by the sort is current\n", in); return 0; }
		}
	}
	const int fd = open_in(in);
	bgzf_in_t bi(fd, threads); bam_hdr_t h;
	if (!hdr_read(bi, h)) die("index: not a BAM file");
	if (env_is_1("SSG_INDEX_DEVICE")) {   /* the records are found on the device; the host loop below takes over, from the start, when that cannot be */
		std::string why;
		if (index_device(in, fd, (int)h.names.size(), bi.tell(), why)) return 0;
		if (dbg()) fprintf(stderr, "[sambamba] index: device index off (%s): the file is walked on the host\n", why.c_str());
	}
	bai_t idx((int)h.names.size(), bi.tell());
	std::vector<uint8_t> rec;
	for (;;) {   /* only the fixed fields, the name and the CIGAR of a record are looked at: the rest (sequence, qualities, tags) is skipped in place */
		uint32_t bs;
		if (bi.get(&bs, 4) != 4) break;
		if (bs < 32) die("index: malformed BAM record");
		rec.resize(32);
		if (bi.get(rec.data(), 32) != 32) die("index: truncated BAM");
		bam_core_t c; memcpy(&c, rec.data(), 32);
		const size_t var = (size_t)(c.bin_mq_nl & 0xff) + 4 * (size_t)(c.flag_nc & 0xffff);
		if (32 + var > bs) die("index: malformed BAM record");
		rec.resize(32 + var);
		if (bi.get(rec.data() + 32, var) != var || bi.skip(bs - 32 - var) != bs - 32 - var) die("index: truncated BAM");
		if (idx.push(c.tid, c.pos, bam_endpos(rec.data()), bi.tell(), !((c.flag_nc >> 16) & 4)) < 0) die("index: the file is not coordinate-sorted");
	}
	idx.finish(bi.tell());
	idx.save((std::string(in) + ".bai").c_str());
	return 0;
}

/* index of a file joined from the parts that the ranks of bin/speedseq-ranks wrote (ranks.h): every rank left, for each record of its part, the
 * fields an index entry is made of and the record's virtual offset in the part; `shift` moves a part's offsets to where its blocks lie in the
 * joined file.  The same bai_t calls in the same order as cmd_index makes from the file itself -- without inflating it again. */
static int cmd_index_parts(int argc, char **argv)
{
	if (argc < 3 || (argc - 1) % 2) die("usage: sambamba index-parts <joined.bam> <part.ssg_ent> <shift> [...]");
	const char *in = argv[0];
	const int fd = open_in(in);
	bgzf_in_t bi(fd, 2); bam_hdr_t h;
	if (!hdr_read(bi, h)) die("index-parts: not a BAM file");
	const uint64_t first = bi.tell();
	struct stat sb; if (fstat(fd, &sb) != 0) die("index-parts: cannot stat the file");
	const uint64_t eof_v = (uint64_t)sb.st_size << 16;
	bai_t idx((int)h.names.size(), first);
	bool have = false; int32_t e_tid = 0, e_pos = 0, e_end = 0; uint32_t e_m = 0;
	std::vector<uint8_t> buf((size_t)24 << 16);
	for (int a = 1; a + 1 < argc; a += 2) {
		const long long shift = atoll(argv[a + 1]);
		FILE *f = fopen(argv[a], "rb"); if (!f) die(std::string("index-parts: cannot read ") + argv[a]);
		for (;;) {
			const size_t k = fread(buf.data(), 24, buf.size() / 24, f);
			if (!k) break;
			for (size_t i = 0; i < k; ++i) {
				const uint8_t *d = buf.data() + 24 * i; uint64_t v; memcpy(&v, d + 16, 8);
				v = (uint64_t)((long long)(v >> 16) + shift) << 16 | (v & 0xffff);
				if (have && idx.push(e_tid, e_pos, e_end, v, e_m != 0) < 0) die("index-parts: the parts are not in coordinate order");
				memcpy(&e_tid, d, 4); memcpy(&e_pos, d + 4, 4); memcpy(&e_end, d + 8, 4); memcpy(&e_m, d + 12, 4); have = true;
			}
		}
		fclose(f);
	}
	if (have && idx.push(e_tid, e_pos, e_end, eof_v, e_m != 0) < 0) die("index-parts: the parts are not in coordinate order");
	idx.finish(eof_v);
	idx.save((std::string(in) + ".bai").c_str());
	close(fd);
	return 0;
}

/* ---------------- merge ---------------- */
static int cmd_merge(int argc, char **argv)
{
	int threads = hw_threads(), level = -1; std::vector<const char*> files;
	for (int i = 0; i < argc; ++i) {
		if (!strcmp(argv[i], "-t") && i + 1 < argc) threads = atoi(argv[++i]);
		else if (!strcmp(argv[i], "-l") && i + 1 < argc) level = atoi(argv[++i]);
		else if (argv[i][0] == '-' && argv[i][1]) die(std::string("merge: unsupported option ") + argv[i]);
		else files.push_back(argv[i]);
	}
	if (files.size() < 2) die("usage: sambamba merge [-t N] out.bam in1.bam [in2.bam ...]");
	std::vector<merge_src_t> src(files.size() - 1);
	for (size_t i = 0; i < src.size(); ++i) { src[i].fd = open_in(files[i + 1]); src[i].in.reset(new bgzf_in_t(src[i].fd, 2)); if (!hdr_read(*src[i].in, src[i].h)) die(std::string("merge: not a BAM file: ") + files[i + 1]); }
	/* header: the first file's, plus the @RG / @PG / @CO lines of the others that it does not hold yet; the references must agree */
	bam_hdr_t h = src[0].h;
	for (size_t i = 1; i < src.size(); ++i) {
		if (src[i].h.names != h.names || src[i].h.lens != h.lens) die("merge: the inputs have different reference sequences");
		size_t p = 0; const std::string &t = src[i].h.text;
		while (p < t.size()) {
			size_t e = t.find('\n', p); if (e == std::string::npos) e = t.size();
			const std::string line = t.substr(p, e - p);
			if (line.size() > 3 && (!line.compare(0, 3, "@RG") || !line.compare(0, 3, "@PG") || !line.compare(0, 3, "@CO")) && ("\n" + h.text).find("\n" + line + "\n") == std::string::npos) h.text += line + "\n";
			p = e + 1;
		}
	}
	if (env_is_1("SSG_MERGE_DEVICE")) {   /* order, gather and deflate on the device, the index written with the file; the host merge below takes over when that cannot be */
		std::string why;
		{ int dl = level; const char *e = getenv("SSG_BAM_LEVEL"); if (dl < 0 && e && *e) dl = atoi(e); if (dl != 0) bgzf_dev_level_set(dl); }   /* SSG_BGZF_DEVICE_LEVELS=1: -l, else SSG_BAM_LEVEL, else 6 */
		if (merge_device(files, src, h, level, threads, why)) return 0;
		if (dbg()) fprintf(stderr, "[sambamba] merge: device merge off (%s): the inputs are merged on the host\n", why.c_str());
	}
	int ofd = open(files[0], O_WRONLY | O_CREAT | O_TRUNC, 0644); if (ofd < 0) die(std::string("merge: cannot write ") + files[0]);
	bgzf_out_t out(ofd, level, threads); hdr_write(out, h);
	kway_merge(src, out); out.finish(); close(ofd);
	return 0;
}

/* ---------------- depth: per-base, region and window coverage, counted on the device (ssg_depth_*, include/ssgpu.h) ----------------
 * What is read: as `view' -- the whole file, or with regions / -L the chunks the .bai gives for them -- in batches of whole members that go into the record store.
 * The targets (the merged regions, or every contig in header order) are cut into spans of at most SSG_DEPTH_SPAN positions, neighbouring small targets of a
 * contig sharing one.  The spans are taken in order: the batches still held are pushed into the span, then batches are loaded and pushed until one holds a record
 * that begins behind the span (n_behind > 0: the file is sorted, no later batch adds to it); a batch with n_later > 0 is held for the next span, the others are
 * released.  A window or BED line that several spans share is summed over them on the host.  There is no host path. */
struct depth_item_t { int32_t tid; int64_t beg, end, pbeg, pend; uint64_t v[2 + 8]; };   /* what is summed (inside its contig) and what is printed */
struct depth_batch_t { uint32_t cid; std::vector<uint64_t> hint; uint64_t first; };
static int cmd_depth(int argc, char **argv)
{
	const char *const usage = "usage: sambamba depth base|region|window [-t N] [-F FILTER] [-q MINBASEQ] [-a] [-T N ...] [-w SIZE] [-L BED] [-o FILE] <in.bam> [region ...]";
	if (argc < 1) die(usage);
	const std::string mode = argv[0];
	if (mode != "base" && mode != "region" && mode != "window") die(std::string("depth: unknown mode `") + mode + "' (base, region, window)");
	const char *expr = "not (unmapped or secondary_alignment or failed_quality_control or duplicate)", *out_path = 0, *bed = 0, *in = 0;
	int min_baseq = 0; bool all = false; int64_t wsize = 0; std::vector<uint32_t> thr; std::vector<std::string> region;
	for (int i = 1; i < argc; ++i) {
		const char *a = argv[i];
		if (!strcmp(a, "-t") && i + 1 < argc) ++i;   /* (the work is the device's) */
		else if (!strcmp(a, "-F") && i + 1 < argc) expr = argv[++i];
		else if (!strcmp(a, "-q") && i + 1 < argc) { int64_t q; if (!view_number(argv[++i], q) || q > 255) die("depth: -q takes a number in 0 .. 255"); min_baseq = (int)q; }
		else if (!strcmp(a, "-a") && mode == "base") all = true;
		else if (!strcmp(a, "-T") && i + 1 < argc && mode != "base") { int64_t t; if (!view_number(argv[++i], t) || t > 0xffffffffll) die("depth: -T takes a number below 2^32"); if (thr.size() == 8) die("depth: at most 8 -T"); thr.push_back((uint32_t)t); }
		else if (!strcmp(a, "-w") && i + 1 < argc && mode == "window") { if (!view_number(argv[++i], wsize) || wsize < 1) die("depth: -w takes a window size of at least 1"); }
		else if (!strcmp(a, "-L") && i + 1 < argc) bed = argv[++i];
		else if (!strcmp(a, "-o") && i + 1 < argc) out_path = argv[++i];
		else if (a[0] == '-' && a[1]) die(std::string("depth ") + mode + ": unsupported option " + a);
		else if (!in) in = a;
		else region.push_back(a);
	}
	if (!in) die(usage);
	if (mode == "window" && wsize < 1) die("depth window: -w SIZE is required");
	if (mode == "region" && !bed) die("depth region: -L BED is required");
	if (mode == "region" && !region.empty()) die("depth region: the regions are the lines of -L");
	view_filter_t filter; filter.compile(expr);
	const int fd = open_in(in);
	std::string why;
	if (!dev_read_ready(fd, why)) die("depth: " + why + " (the coverage is counted on the device; there is no host path)");
	bam_hdr_t h;
	uint64_t v0 = 0;
	{ bgzf_in_t bi(fd, 1); if (!hdr_read(bi, h)) die("depth: not a BAM file"); v0 = bi.tell(); }
	/* the targets: merged regions inside their contigs, or every contig */
	std::vector<ssg_bam_region_t> reg, lines;
	for (const std::string &r : region) view_region_add(h, r, reg);
	if (bed) { view_bed_read(h, bed, lines); reg.insert(reg.end(), lines.begin(), lines.end()); }
	const bool with_regions = bed || !region.empty();
	view_regions_merge(reg);
	if (!with_regions) for (size_t t = 0; t < h.names.size(); ++t) { ssg_bam_region_t r; r.tid = (int32_t)t; r.beg = 0; r.end = h.lens[t]; reg.push_back(r); }
	std::vector<ssg_bam_region_t> targets;
	for (ssg_bam_region_t r : reg) { r.end = std::min(r.end, h.lens[(size_t)r.tid]); if (r.beg < r.end) targets.push_back(r); }
	/* what region and window print, in their order */
	std::vector<depth_item_t> items;
	auto item_add = [&](int32_t tid, int64_t b, int64_t e) { depth_item_t it; memset(&it, 0, sizeof(it)); it.tid = tid; it.pbeg = b; it.pend = e; it.beg = b; it.end = std::min<int64_t>(e, h.lens[(size_t)tid]); items.push_back(it); };
	if (mode == "region") for (const ssg_bam_region_t &l : lines) item_add(l.tid, l.beg, l.end);
	if (mode == "window") for (const ssg_bam_region_t &t : targets) for (int64_t b = t.beg; b < t.end; b += wsize) item_add(t.tid, b, std::min<int64_t>(b + wsize, t.end));
	std::vector<std::vector<size_t> > items_of(h.names.size());
	for (size_t k = 0; k < items.size(); ++k) items_of[(size_t)items[k].tid].push_back(k);
	/* the spans */
	const char *const se = getenv("SSG_DEPTH_SPAN");
	const int64_t SPAN = std::max<int64_t>(1, std::min<int64_t>(se && *se ? strtoll(se, 0, 10) : (int64_t)1 << 26, (int64_t)1 << 28));
	struct span_t { int32_t tid; int64_t beg, end; std::vector<ssg_bam_region_t> parts; };
	std::vector<span_t> spans;
	for (const ssg_bam_region_t &t : targets)
		for (int64_t b = t.beg; b < t.end; b += SPAN) {
			ssg_bam_region_t p; p.tid = t.tid; p.beg = (int32_t)b; p.end = (int32_t)std::min<int64_t>(b + SPAN, t.end);
			if (spans.empty() || spans.back().tid != p.tid || p.end - spans.back().beg > SPAN) { span_t s; s.tid = p.tid; s.beg = p.beg; spans.push_back(s); }
			spans.back().end = p.end; spans.back().parts.push_back(p);
		}
	/* what to read */
	dev_batches_t R;
	if (with_regions) bai_chunks_for("depth", in, fd, h.names.size(), targets, R.chunks);
	else R.whole_file(v0);
	int out_fd = 1;
	if (out_path) { out_fd = open(out_path, O_WRONLY | O_CREAT | O_TRUNC, 0666); if (out_fd < 0) die(std::string("cannot write ") + out_path + ": " + strerror(errno)); g_partial_out = out_path; }
	recs_holder_t S;
	struct depth_holder_t { ssg_depth_t *d; ~depth_holder_t() { if (d) ssg_depth_free(d); } } D = { 0 };   /* (freed before the store: declared behind it) */
	if (ssg_set_device(0) || ssg_recs_create(~(uint64_t)0 >> 1, &S.r)) die(std::string("depth: ") + ssg_last_error());
	if (ssg_depth_create(S.r, filter.prog.data(), (int)filter.prog.size(), min_baseq, &D.d)) die(std::string("depth: ") + ssg_last_error());
	dev_prof_begin();
	/* the reader: the next batch of the chunk list, kept while a later span needs it */
	R.init("depth", S.r, fd, in, (uint64_t)64 << 20, 1024);
	auto load = [&](depth_batch_t &B) -> bool {
		const int got = R.next();
		if (got == DEV_FAIL) die("depth: " + R.why);
		if (got == DEV_BATCH) { B.cid = R.cid; B.hint = R.hint; B.first = R.first; }
		return got == DEV_BATCH;
	};
	std::vector<depth_batch_t> held; bool behind = false; uint64_t used = 0;
	auto push = [&](depth_batch_t &B) {
		uint64_t n_rec = 0, n_used = 0, n_later = 0, desc = 0, n_behind = 0;
		const int rc = ssg_depth_push(D.d, B.cid, B.hint.data(), (int64_t)B.hint.size() - 1, B.first, &n_rec, &n_used, &n_later, &desc, &n_behind);
		if (rc) die("depth: " + dev_stage_error(rc, in, "ssg_depth_push: "));
		if (desc) die(std::string("depth: ") + in + " is not sorted by coordinate (" + std::to_string(desc) + " records lie before their predecessor): sambamba sort first");
		used += n_used; behind = behind || n_behind > 0;
		if (n_later > 0) return true;
		if (ssg_recs_release(S.r, B.cid)) die(std::string("depth: ") + ssg_last_error());
		return false;
	};
	const size_t TEXT_N = (size_t)1 << 22;   /* positions of one ssg_depth_text */
	std::vector<uint8_t> text; std::vector<int64_t> pairs; std::vector<size_t> pair_item; std::vector<uint64_t> sums;
	for (const span_t &s : spans) {
		if (ssg_depth_begin(D.d, s.tid, s.beg, s.end)) die(std::string("depth: ") + ssg_last_error());
		behind = false; used = 0;
		std::vector<depth_batch_t> keep;
		for (depth_batch_t &B : held) if (push(B)) keep.push_back(std::move(B));
		held.swap(keep);
		depth_batch_t B;
		while (!behind && load(B)) if (push(B)) held.push_back(std::move(B));
		if (mode == "base" && !all && used == 0) { if (ssg_depth_end(D.d)) die(std::string("depth: ") + ssg_last_error()); continue; }
		if (ssg_depth_finish(D.d)) die(std::string("depth: ") + ssg_last_error());
		const std::string &name = h.names[(size_t)s.tid];
		if (mode == "base") {
			text.resize(std::min<size_t>(TEXT_N, (size_t)(s.end - s.beg)) * (name.size() + 23));   /* (a line: the name, two tabs, a newline, two numbers of at most ten digits) */
			for (const ssg_bam_region_t &p : s.parts)
				for (int64_t b = p.beg; b < p.end; b += (int64_t)TEXT_N) {
					uint64_t len = 0;
					if (ssg_depth_text(D.d, name.c_str(), b, std::min<int64_t>(b + (int64_t)TEXT_N, p.end), all ? 1 : 0, text.data(), text.size(), &len)) die(std::string("depth: ") + ssg_last_error());
					io_write_all(out_fd, text.data(), (size_t)len);
				}
		} else {
			pairs.clear(); pair_item.clear();
			for (size_t k : items_of[(size_t)s.tid]) {
				const int64_t b = std::max(items[k].beg, s.beg), e = std::min(items[k].end, s.end);
				if (b < e) { pairs.push_back(b); pairs.push_back(e); pair_item.push_back(k); }
			}
			const size_t row = 2 + thr.size();
			sums.assign(pair_item.size() * row + 1, 0);
			if (ssg_depth_sums(D.d, pairs.data(), (int64_t)pair_item.size(), thr.data(), (int)thr.size(), sums.data())) die(std::string("depth: ") + ssg_last_error());
			for (size_t j = 0; j < pair_item.size(); ++j) for (size_t c = 0; c < row; ++c) items[pair_item[j]].v[c] += sums[j * row + c];
		}
		if (ssg_depth_end(D.d)) die(std::string("depth: ") + ssg_last_error());
	}
	if (mode != "base") {
		std::string out;
		for (const depth_item_t &it : items) {
			char num[64];
			out += h.names[(size_t)it.tid]; out += '\t'; out += std::to_string(it.pbeg); out += '\t'; out += std::to_string(it.pend); out += '\t';
			out += std::to_string(it.v[0]); out += '\t'; out += std::to_string(it.v[1]);
			snprintf(num, sizeof(num), "\t%.4f", (double)it.v[1] / (double)(it.pend - it.pbeg)); out += num;
			for (size_t c = 0; c < thr.size(); ++c) { out += '\t'; out += std::to_string(it.v[2 + c]); }
			out += '\n';
			if (out.size() > ((size_t)1 << 20)) { io_write_all(out_fd, out.data(), out.size()); out.clear(); }
		}
		io_write_all(out_fd, out.data(), out.size());
	}
	dev_prof_report("sambamba", "depth");
	g_partial_out = 0; if (out_path) close(out_fd);
	return 0;
}

/* ---------------- stats: the QC tables of `samtools stats', counted on the device (ssg_stats_*, include/ssgpu.h) ----------------
 * The whole file is read in batches of whole members that go into the record store; every batch is pushed and released.  What is printed is output_stats of
 * samtools 1.3.1 stats.c, line for line and section comment for section comment, behind two comment lines of this program's own: CHK, the 31 SN lines, FFQ, LFQ,
 * GCF, GCL, GCC, IS, RL, ID, IC and COV.  The five float lines restate the C expressions with their types.  GCD is not computed (a comment line says so), and an
 * unsorted file gets a comment in place of its COV rows.  There is no host path. */
static void stats_put(std::string &out, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
static void stats_put(std::string &out, const char *fmt, ...)
{
	char buf[512]; va_list ap; va_start(ap, fmt); const int n = vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
	if (n > 0) out.append(buf, std::min<size_t>((size_t)n, sizeof(buf) - 1));
}
static int cmd_stats(int argc, char **argv)
{
	const char *const usage = "usage: sambamba stats [-t N] [-F FILTER] [-c MIN,MAX,STEP] [-i N] [-m FRAC] [-x] [--max-read-length N] <in.bam>";
	const char *expr = 0, *in = 0; bool sparse = false; float main_bulk = 0.99f;   /* (isize_main_bulk is a float in stats_info_t) */
	ssg_stats_opt_t o; o.max_len = 1024; o.n_isize = 8000; o.cov_min = 1; o.cov_max = 1000; o.cov_step = 1; o.span = 0;
	for (int i = 0; i < argc; ++i) {
		const char *a = argv[i];
		if (!strcmp(a, "-t") && i + 1 < argc) ++i;   /* (the work is the device's) */
		else if (!strcmp(a, "-F") && i + 1 < argc) expr = argv[++i];
		else if (!strcmp(a, "-c") && i + 1 < argc) { if (sscanf(argv[++i], "%d,%d,%d", &o.cov_min, &o.cov_max, &o.cov_step) != 3) die("stats: -c takes MIN,MAX,STEP"); }
		else if (!strcmp(a, "-i") && i + 1 < argc) { int64_t v; if (!view_number(argv[++i], v) || v < 1 || v > (1 << 24)) die("stats: -i takes a number in 1 .. 2^24"); o.n_isize = (int32_t)v; }
		else if (!strcmp(a, "-m") && i + 1 < argc) main_bulk = (float)atof(argv[++i]);
		else if (!strcmp(a, "-x")) sparse = true;
		else if (!strcmp(a, "--max-read-length") && i + 1 < argc) { int64_t v; if (!view_number(argv[++i], v) || v < 1 || v > 65535) die("stats: --max-read-length takes a number in 1 .. 65535"); o.max_len = (int32_t)v; }
		else if (a[0] == '-' && a[1]) die(std::string("stats: unsupported option ") + a);
		else if (!in) in = a;
		else die("stats: one input file (regions are not supported)");
	}
	if (!in) die(usage);
	view_filter_t filter; if (expr) filter.compile(expr);
	const char *const sp = getenv("SSG_STATS_SPAN");
	if (sp && *sp) o.span = (int32_t)std::max<long long>(1, std::min<long long>(strtoll(sp, 0, 10), 1 << 28));
	const int64_t n_cov = ssg_stats_ncov(&o);
	if (n_cov < 0) die("stats: -c takes 0 <= MIN <= MAX <= 16777216 and STEP >= 1, with at most 8192 bins");
	const int fd = open_in(in);
	std::string why;
	if (!dev_read_ready(fd, why)) die("stats: " + why + " (the tables are counted on the device; there is no host path)");
	bam_hdr_t h; uint64_t v0 = 0;
	{ bgzf_in_t bi(fd, 1); if (!hdr_read(bi, h)) die("stats: not a BAM file"); v0 = bi.tell(); }
	recs_holder_t S;
	struct stats_holder_t { ssg_stats_t *s; ~stats_holder_t() { if (s) ssg_stats_free(s); } } T = { 0 };   /* (freed before the store: declared behind it) */
	if (ssg_set_device(0) || ssg_recs_create(~(uint64_t)0 >> 1, &S.r)) die(std::string("stats: ") + ssg_last_error());
	if (ssg_stats_create(S.r, filter.prog.data(), (int)filter.prog.size(), &o, &T.s)) die(std::string("stats: ") + ssg_last_error());
	dev_prof_begin();
	dev_batches_t R; R.init("stats", S.r, fd, in, (uint64_t)64 << 20, 1024); R.whole_file(v0);
	for (;;) {
		const int got = R.next();
		if (got == DEV_FAIL) die("stats: " + R.why);
		if (got != DEV_BATCH) break;
		uint64_t n_rec = 0, desc = 0;
		const int rc = ssg_stats_push(T.s, R.cid, R.hint.data(), (int64_t)R.hint.size() - 1, R.first, &n_rec, &desc);
		if (rc) die("stats: " + dev_stage_error(rc, in, "ssg_stats_push: "));
		if (ssg_recs_release(S.r, R.cid)) die(std::string("stats: ") + ssg_last_error());
	}
	if (ssg_stats_finish(T.s)) die(std::string("stats: ") + ssg_last_error());
	const size_t rows = (size_t)o.max_len + 1, ni = (size_t)o.n_isize;
	std::vector<uint64_t> sc(SSG_ST_N), quals(2 * rows * 256), acgt(rows * 6), gc(2 * SSG_STATS_NGC), isz(3 * ni), rl(rows), id(2 * SSG_STATS_NINDEL), ic(4 * rows), cov((size_t)n_cov);
	if (ssg_stats_get(T.s, sc.data(), quals.data(), acgt.data(), gc.data(), isz.data(), rl.data(), id.data(), ic.data(), cov.data())) die(std::string("stats: ") + ssg_last_error());
	dev_prof_report("sambamba", "stats");
	/* output_stats: the insert sizes first (each pair was counted twice; ssg_stats_get has halved them) */
	const uint64_t *const in_ = isz.data(), *const out_ = in_ + ni, *const oth_ = out_ + ni;
	int ibulk = 0; uint64_t nisize = 0, n_in = 0, n_out = 0, n_oth = 0;
	for (size_t k = 0; k < ni; ++k) { n_in += in_[k]; n_out += out_[k]; n_oth += oth_[k]; nisize += in_[k] + out_[k] + oth_[k]; }
	double bulk = 0, avg_isize = 0, sd_isize = 0;
	for (int k = 0; k < (int)ni; ++k) {
		bulk += in_[k] + out_[k] + oth_[k];
		avg_isize += k * (in_[k] + out_[k] + oth_[k]);
		if (bulk / nisize > main_bulk) { ibulk = k + 1; nisize = bulk; break; }
	}
	avg_isize /= nisize ? nisize : 1;
	for (int k = 1; k < ibulk; ++k) sd_isize += (in_[k] + out_[k] + oth_[k]) * (k - avg_isize) * (k - avg_isize) / nisize;
	sd_isize = sqrt(sd_isize);
	const uint64_t n1 = sc[SSG_ST_FIRST], n2 = sc[SSG_ST_LAST], total_len = sc[SSG_ST_TOTAL_LEN], mism = sc[SSG_ST_MISMATCHES], cig = sc[SSG_ST_BASES_CIGAR];
	const double sum_qual = (double)sc[SSG_ST_SUM_QUAL];
	int max_len = std::max<int>(30, (int)sc[SSG_ST_MAX_LEN]), max_qual = std::max<int>(40, (int)sc[SSG_ST_MAX_QUAL]);   /* stats_init's starting values */
	std::string t;
	auto flush = [&](bool all) { if (all || t.size() > ((size_t)1 << 20)) { io_write_all(1, t.data(), t.size()); t.clear(); } };
	stats_put(t, "# This file was produced by sambamba stats (libssgpu %s, %s) in the layout of samtools stats 1.3.1 and can be plotted using plot-bamstats\n", ssg_version(), ssg_backend());
	stats_put(t, "# This file contains statistics for all reads.\n");
	t += std::string("# The input was:  ") + in + (expr ? std::string("  filtered by:  ") + expr : std::string()) + "\n";
	stats_put(t, "# CHK, Checksum\t[2]Read Names\t[3]Sequences\t[4]Qualities\n");
	stats_put(t, "# CHK, CRC32 of reads which passed filtering followed by addition (32bit overflow)\n");
	stats_put(t, "CHK\t%08x\t%08x\t%08x\n", (unsigned)sc[SSG_ST_CHK_NAMES], (unsigned)sc[SSG_ST_CHK_READS], (unsigned)sc[SSG_ST_CHK_QUALS]);
	stats_put(t, "# Summary Numbers. Use `grep ^SN | cut -f 2-` to extract this part.\n");
	stats_put(t, "SN\traw total sequences:\t%ld\n", (long)(sc[SSG_ST_FILTERED] + n1 + n2));
	stats_put(t, "SN\tfiltered sequences:\t%ld\n", (long)sc[SSG_ST_FILTERED]);
	stats_put(t, "SN\tsequences:\t%ld\n", (long)(n1 + n2));
	stats_put(t, "SN\tis sorted:\t%d\n", sc[SSG_ST_SORTED] ? 1 : 0);
	stats_put(t, "SN\t1st fragments:\t%ld\n", (long)n1);
	stats_put(t, "SN\tlast fragments:\t%ld\n", (long)n2);
	stats_put(t, "SN\treads mapped:\t%ld\n", (long)(sc[SSG_ST_PAIRED_MAPPED] + sc[SSG_ST_SINGLE]));
	stats_put(t, "SN\treads mapped and paired:\t%ld\t# paired-end technology bit set + both mates mapped\n", (long)sc[SSG_ST_PAIRED_MAPPED]);
	stats_put(t, "SN\treads unmapped:\t%ld\n", (long)sc[SSG_ST_UNMAPPED]);
	stats_put(t, "SN\treads properly paired:\t%ld\t# proper-pair bit set\n", (long)sc[SSG_ST_PROPER]);
	stats_put(t, "SN\treads paired:\t%ld\t# paired-end technology bit set\n", (long)sc[SSG_ST_PAIRED]);
	stats_put(t, "SN\treads duplicated:\t%ld\t# PCR or optical duplicate bit set\n", (long)sc[SSG_ST_DUP]);
	stats_put(t, "SN\treads MQ0:\t%ld\t# mapped and MQ=0\n", (long)sc[SSG_ST_MQ0]);
	stats_put(t, "SN\treads QC failed:\t%ld\n", (long)sc[SSG_ST_QCFAIL]);
	stats_put(t, "SN\tnon-primary alignments:\t%ld\n", (long)sc[SSG_ST_SECONDARY]);
	stats_put(t, "SN\ttotal length:\t%ld\t# ignores clipping\n", (long)total_len);
	stats_put(t, "SN\tbases mapped:\t%ld\t# ignores clipping\n", (long)sc[SSG_ST_BASES_MAPPED]);
	stats_put(t, "SN\tbases mapped (cigar):\t%ld\t# more accurate\n", (long)cig);
	stats_put(t, "SN\tbases trimmed:\t%ld\n", 0l);
	stats_put(t, "SN\tbases duplicated:\t%ld\n", (long)sc[SSG_ST_DUP_LEN]);
	stats_put(t, "SN\tmismatches:\t%ld\t# from NM fields\n", (long)mism);
	stats_put(t, "SN\terror rate:\t%e\t# mismatches / bases mapped (cigar)\n", cig ? (float)mism / cig : 0);   /* a float quotient, as the C expression has it */
	const float avg_read_length = (n1 + n2) ? total_len / (n1 + n2) : 0;   /* an integer quotient */
	stats_put(t, "SN\taverage length:\t%.0f\n", avg_read_length);
	stats_put(t, "SN\tmaximum length:\t%d\n", max_len);
	stats_put(t, "SN\taverage quality:\t%.1f\n", total_len ? sum_qual / total_len : 0);
	stats_put(t, "SN\tinsert size average:\t%.1f\n", avg_isize);
	stats_put(t, "SN\tinsert size standard deviation:\t%.1f\n", sd_isize);
	stats_put(t, "SN\tinward oriented pairs:\t%ld\n", (long)n_in);
	stats_put(t, "SN\toutward oriented pairs:\t%ld\n", (long)n_out);
	stats_put(t, "SN\tpairs with other orientation:\t%ld\n", (long)n_oth);
	stats_put(t, "SN\tpairs on different chromosomes:\t%ld\n", (long)sc[SSG_ST_ANOMALOUS] / 2);
	if (max_len < (int)rows) max_len++;
	if (max_qual + 1 < 256) max_qual++;
	for (int f = 0; f < 2; ++f) {
		stats_put(t, "# %s Fragment Qualitites. Use `grep ^%s | cut -f 2-` to extract this part.\n", f ? "Last" : "First", f ? "LFQ" : "FFQ");
		stats_put(t, "# Columns correspond to qualities and rows to cycles. First column is the cycle number.\n");
		for (int b = 0; b < max_len && b < (int)rows; ++b) {
			stats_put(t, "%s\t%d", f ? "LFQ" : "FFQ", b + 1);
			for (int q = 0; q <= max_qual; ++q) stats_put(t, "\t%ld", (long)quals[((size_t)f * rows + (size_t)b) * 256 + (size_t)q]);
			t += '\n'; flush(false);
		}
	}
	for (int f = 0; f < 2; ++f) {
		stats_put(t, "# GC Content of %s fragments. Use `grep ^%s | cut -f 2-` to extract this part.\n", f ? "last" : "first", f ? "GCL" : "GCF");
		const uint64_t *g = gc.data() + (size_t)f * SSG_STATS_NGC; int prev = 0;
		for (int b = 0; b < SSG_STATS_NGC; ++b) {
			if (g[b] == g[prev]) continue;
			stats_put(t, "%s\t%.2f\t%ld\n", f ? "GCL" : "GCF", (b + prev) * 0.5 * 100. / (SSG_STATS_NGC - 1), (long)g[prev]);
			prev = b;
		}
	}
	stats_put(t, "# ACGT content per cycle. Use `grep ^GCC | cut -f 2-` to extract this part. The columns are: cycle; A,C,G,T base counts as a percentage of all A/C/G/T bases [%%]; and N and O counts as a percentage of all A/C/G/T bases [%%]\n");
	for (int b = 0; b < max_len && b < (int)rows; ++b) {
		const uint64_t *c = acgt.data() + (size_t)b * 6; const uint64_t sum = c[0] + c[1] + c[2] + c[3];
		if (!sum) continue;
		stats_put(t, "GCC\t%d\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f\t%.2f\n", b + 1, 100. * c[0] / sum, 100. * c[1] / sum, 100. * c[2] / sum, 100. * c[3] / sum, 100. * c[4] / sum, 100. * c[5] / sum);
	}
	stats_put(t, "# Insert sizes. Use `grep ^IS | cut -f 2-` to extract this part. The columns are: insert size, pairs total, inward oriented pairs, outward oriented pairs, other pairs\n");
	for (int k = 0; k < ibulk; ++k) {
		const long a = (long)in_[k], b = (long)out_[k], c = (long)oth_[k];
		if (!sparse || a + b + c > 0) stats_put(t, "IS\t%d\t%ld\t%ld\t%ld\t%ld\n", k, a + b + c, a, b, c);
		flush(false);
	}
	stats_put(t, "# Read lengths. Use `grep ^RL | cut -f 2-` to extract this part. The columns are: read length, count\n");
	for (int k = 0; k < max_len && k < (int)rows; ++k) if (rl[(size_t)k] > 0) stats_put(t, "RL\t%d\t%ld\n", k, (long)rl[(size_t)k]);
	stats_put(t, "# Indel distribution. Use `grep ^ID | cut -f 2-` to extract this part. The columns are: length, number of insertions, number of deletions\n");
	for (int k = 0; k < SSG_STATS_NINDEL; ++k) if (id[(size_t)k] > 0 || id[SSG_STATS_NINDEL + (size_t)k] > 0) stats_put(t, "ID\t%d\t%ld\t%ld\n", k + 1, (long)id[(size_t)k], (long)id[SSG_STATS_NINDEL + (size_t)k]);
	stats_put(t, "# Indels per cycle. Use `grep ^IC | cut -f 2-` to extract this part. The columns are: cycle, number of insertions (fwd), .. (rev) , number of deletions (fwd), .. (rev)\n");
	for (size_t k = 0; k < rows; ++k)
		if (ic[k] > 0 || ic[rows + k] > 0 || ic[2 * rows + k] > 0 || ic[3 * rows + k] > 0) stats_put(t, "IC\t%d\t%ld\t%ld\t%ld\t%ld\n", (int)k + 1, (long)ic[k], (long)ic[rows + k], (long)ic[2 * rows + k], (long)ic[3 * rows + k]);
	stats_put(t, "# Coverage distribution. Use `grep ^COV | cut -f 2-` to extract this part.\n");
	if (!sc[SSG_ST_SORTED]) stats_put(t, "# COV is not computed: the file is not sorted by coordinate\n");
	else {
		int step = o.cov_step;   /* as init_stat_structs rounds it */
		if (step > o.cov_max - o.cov_min + 1) { step = o.cov_max - o.cov_min; if (step <= 0) step = 1; }
		if (cov[0]) stats_put(t, "COV\t[<%d]\t%d\t%ld\n", o.cov_min, o.cov_min - 1, (long)cov[0]);
		for (int k = 1; k < (int)n_cov - 1; ++k)
			if (cov[(size_t)k]) stats_put(t, "COV\t[%d-%d]\t%d\t%ld\n", o.cov_min + (k - 1) * step, o.cov_min + k * step - 1, o.cov_min + k * step - 1, (long)cov[(size_t)k]);
		if (cov[(size_t)n_cov - 1]) stats_put(t, "COV\t[%d<]\t%d\t%ld\n", o.cov_min + ((int)n_cov - 2) * step - 1, o.cov_min + ((int)n_cov - 2) * step - 1, (long)cov[(size_t)n_cov - 1]);
	}
	stats_put(t, "# GC-depth. Use `grep ^GCD | cut -f 2-` to extract this part. The columns are: GC%%, unique sequence percentiles, 10th, 25th, 50th, 75th and 90th depth percentile\n");
	stats_put(t, "# GCD is not computed\n");
	flush(true);
	return 0;
}

/* ---------------- markdup: Picard's duplicate rule, decided on the device (ssg_markdup_*, include/ssgpu.h) ----------------
 * The file is read twice, each time in batches of whole members that go into the record store.  The first pass pushes every batch (ssg_markdup_push leaves an
 * entry per record on the device and releases the batch) and decides (ssg_markdup_finish); the second patches the flag bytes of a batch in the store and writes
 * its kept records as view_device writes BAM: declared as the stream, cut into blocks by bgzf_out_t::record's rule, gathered, deflated and framed on the device.
 * At -l 0 the batch is gathered to the host and leaves through bgzf_out_t: stored blocks are the host's.  The header is the input's, with no @PG added.
 * --tmpdir, --hash-table-size, --overflow-list-size, --sort-buffer-size, --io-buffer-size and -p are upstream's host-memory and progress knobs: taken and
 * ignored.  SSG_MARKDUP_BATCH: the inflated bytes of a batch (default 64 MB; tests: groups and mates in different batches).  There is no host path. */
static void markdup_libraries(const bam_hdr_t &h, std::vector<std::string> &ids, std::vector<uint16_t> &libs)
{
	std::unordered_map<std::string, uint16_t> lib_id;
	size_t at = 0;
	while (at < h.text.size()) {
		size_t e = h.text.find('\n', at); if (e == std::string::npos) e = h.text.size();
		const std::string line = h.text.substr(at, e - at); at = e + 1;
		if (line.compare(0, 4, "@RG\t") != 0) continue;
		std::string id, lb; bool has_lb = false;
		size_t f = 4;
		while (f <= line.size()) {
			size_t fe = line.find('\t', f); if (fe == std::string::npos) fe = line.size();
			if (line.compare(f, 3, "ID:") == 0) id = line.substr(f + 3, fe - f - 3);
			else if (line.compare(f, 3, "LB:") == 0) { lb = line.substr(f + 3, fe - f - 3); has_lb = true; }
			f = fe + 1;
		}
		if (id.empty()) continue;
		uint16_t l = 0;
		if (has_lb) {
			auto it = lib_id.find(lb);
			if (it == lib_id.end()) {
				if (lib_id.size() >= 65535) die("markdup: more than 65535 libraries in the header");
				it = lib_id.emplace(lb, (uint16_t)(lib_id.size() + 1)).first;
			}
			l = it->second;
		}
		ids.push_back(id); libs.push_back(l);
	}
}
static int cmd_markdup(int argc, char **argv)
{
	const char *const usage = "usage: sambamba markdup [-r] [-t N] [-l LEVEL] [-p] [--tmpdir=DIR] [--hash-table-size=N] [--overflow-list-size=N] [--sort-buffer-size=N] [--io-buffer-size=N] <in.bam> <out.bam>";
	int threads = hw_threads(), level = -1; bool remove = false; const char *in = 0, *outp = 0;
	for (int i = 0; i < argc; ++i) {
		const char *a = argv[i];
		if (!strcmp(a, "-r") || !strcmp(a, "--remove-duplicates")) remove = true;
		else if (!strcmp(a, "-t") && i + 1 < argc) threads = std::max(1, atoi(argv[++i]));
		else if (!strcmp(a, "-l") && i + 1 < argc) level = atoi(argv[++i]);
		else if (!strcmp(a, "-p") || !strcmp(a, "--show-progress")) {}
		else if (!strncmp(a, "--tmpdir=", 9) || !strncmp(a, "--hash-table-size=", 18) || !strncmp(a, "--overflow-list-size=", 21) || !strncmp(a, "--sort-buffer-size=", 19) || !strncmp(a, "--io-buffer-size=", 17)) {}
		else if (a[0] == '-' && a[1]) die(std::string("markdup: unsupported option ") + a);
		else if (!in) in = a;
		else if (!outp) outp = a;
		else die("markdup: one input file and one output file (sambamba merge joins several inputs first)");
	}
	if (!in || !outp) die(usage);
	{ const char *e = getenv("SSG_BAM_LEVEL"); if (level < 0 && e && *e) level = atoi(e); }   /* as sort: zlib's 6 when -l is not given */
	const int fd = open_in(in);
	std::string why;
	if (!dev_read_ready(fd, why)) die("markdup: " + why + " (the file is read twice and decided on the device; there is no host path)");
	bam_hdr_t h; uint64_t v0 = 0;
	{ bgzf_in_t bi(fd, 1); if (!hdr_read(bi, h)) die("markdup: not a BAM file"); v0 = bi.tell(); }
	std::vector<std::string> ids; std::vector<uint16_t> libs; std::vector<const char*> idp;
	markdup_libraries(h, ids, libs);
	for (const std::string &s : ids) idp.push_back(s.c_str());
	const char *const be = getenv("SSG_MARKDUP_BATCH");
	const uint64_t window = be && *be ? std::max<uint64_t>(1, strtoull(be, 0, 10)) : (uint64_t)64 << 20;
	recs_holder_t S;
	struct md_holder_t { ssg_markdup_t *m; ~md_holder_t() { if (m) ssg_markdup_free(m); } } T = { 0 };   /* (freed before the store: declared behind it) */
	if (ssg_set_device(0) || ssg_recs_create(~(uint64_t)0 >> 1, &S.r)) die(std::string("markdup: ") + ssg_last_error());
	if (ssg_markdup_create(S.r, idp.empty() ? 0 : idp.data(), libs.empty() ? 0 : libs.data(), (int)idp.size(), 64, &T.m)) die(std::string("markdup: ") + ssg_last_error());
	dev_prof_begin();
	const double t0 = wall();
	{
		dev_batches_t R; R.init("markdup", S.r, fd, in, window, 1024); R.whole_file(v0);
		for (;;) {
			const int got = R.next();
			if (got == DEV_FAIL) die("markdup: " + R.why);
			if (got != DEV_BATCH) break;
			uint64_t n_rec = 0;
			const int rc = ssg_markdup_push(T.m, R.cid, R.hint.data(), (int64_t)R.hint.size() - 1, R.first, &n_rec);
			if (rc) die("markdup: " + dev_stage_error(rc, in, "ssg_markdup_push: "));
		}
	}
	uint64_t counts[SSG_MD_N];
	if (ssg_markdup_finish(T.m, counts)) die(std::string("markdup: ") + ssg_last_error());
	/* the second pass */
	const int out_fd = open(outp, O_WRONLY | O_CREAT | O_TRUNC, 0644);
	if (out_fd < 0) die(std::string("markdup: cannot write ") + outp);
	g_partial_out = outp;
	const bool stored = level == 0;
	if (!stored) bgzf_dev_level_set(level);
	const long BATCH = 1024;   /* blocks per device call */
	const uint64_t out_cap = stored ? 0 : ssg_bgzf_bound((uint64_t)BATCH * BGZF_MAX_PAYLOAD, BATCH);
	host_pinned_t O;
	if (!stored && !O.grow(out_cap)) die("markdup: no page-locked memory for the output blocks");
	bgzf_out_t ho(out_fd, stored ? 0 : level, threads);   /* the header's blocks; at -l 0 the records' too */
	bool begun = false;
	auto begin = [&]() { if (!begun) { hdr_write(ho, h); if (stored) ho.close_block(); else ho.drain(true); begun = true; g_partial_out = 0; } };
	auto fail = [&](const std::string &m) { die("markdup: " + m + (begun ? " after output had begun" : "")); };
	std::vector<uint64_t> loc, cum, cut, boff((size_t)BATCH + 1); std::vector<ssg_bam_ent_t> ent; std::vector<uint8_t> buf;
	uint64_t n_out = 0;
	{
		dev_batches_t R; R.init("markdup", S.r, fd, in, window, 1024); R.whole_file(v0);
		for (int got; (got = R.next()) != DEV_END; ) {
			if (got == DEV_FAIL) fail(R.why);
			const size_t nm = R.n();
			uint64_t n_rec = 0, n_kept = 0;
			const uint64_t cap = R.hint[nm] / 36 + 1;
			loc.resize((size_t)cap); ent.resize((size_t)cap);
			const int rc = ssg_markdup_apply(T.m, R.cid, R.hint.data(), (int64_t)nm, R.first, remove ? 1 : 0, cap, &n_rec, &n_kept, loc.data(), ent.data());
			if (rc) fail(dev_stage_error(rc, in, "ssg_markdup_apply: "));
			if (n_kept) {
				cum.resize((size_t)n_kept + 1); cum[0] = 0;
				for (uint64_t i = 0; i < n_kept; ++i) cum[(size_t)i + 1] = cum[(size_t)i] + ent[(size_t)i].len;
				if (ssg_recs_order(S.r, loc.data(), cum.data(), (int64_t)n_kept)) fail(ssg_last_error());
				if (stored) {
					buf.resize((size_t)cum[(size_t)n_kept]);
					if (ssg_recs_gather(S.r, 0, cum[(size_t)n_kept], buf.data())) fail(ssg_last_error());
					begin();
					for (uint64_t i = 0; i < n_kept; ++i) ho.record(buf.data() + cum[(size_t)i], (size_t)ent[(size_t)i].len);
				} else {
					bgzf_cut_blocks(cum.data(), (size_t)n_kept, cut);   /* (a batch ends its last block) */
					const size_t nb = cut.size() - 1;
					for (size_t b0 = 0; b0 < nb; b0 += (size_t)BATCH) {
						const long k = (long)std::min<size_t>((size_t)BATCH, nb - b0);
						if (dev_bgzf_compress_recs(S.r, cut.data() + b0, k, O.p, out_cap, boff.data(), 0)) fail(ssg_last_error());
						begin();
						io_write_all(out_fd, O.p, (size_t)boff[(size_t)k]);
					}
				}
				if (ssg_recs_reopen(S.r)) fail(ssg_last_error());
			}
			if (ssg_recs_release(S.r, R.cid)) fail(ssg_last_error());
			n_out += n_kept;
		}
	}
	begin();
	if (stored) ho.finish(); else io_write_all(out_fd, BGZF_EOF, 28);
	close(out_fd);
	fprintf(stderr, "[sambamba] markdup: %llu records, %llu taking part, %llu pairs, %llu unmatched paired, %llu fragments, %llu duplicates found (%llu in pairs, %llu fragments)%s, %llu records written, %.2f s\n",
	        (unsigned long long)counts[SSG_MD_RECORDS], (unsigned long long)counts[SSG_MD_TAKING_PART], (unsigned long long)counts[SSG_MD_PAIRS], (unsigned long long)counts[SSG_MD_UNMATCHED],
	        (unsigned long long)counts[SSG_MD_FRAGMENTS], (unsigned long long)(counts[SSG_MD_DUP_PAIRED] + counts[SSG_MD_DUP_FRAGMENTS]), (unsigned long long)counts[SSG_MD_DUP_PAIRED],
	        (unsigned long long)counts[SSG_MD_DUP_FRAGMENTS], remove ? " and removed" : "", (unsigned long long)n_out, wall() - t0);
	dev_prof_report("sambamba", "markdup");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: sambamba <view|sort|index|merge|flagstat|depth|stats|markdup> ...  (libssgpu %s, %s)\n", ssg_version(), ssg_backend()); return 1; }
#ifdef F_SETPIPE_SZ
	(void)fcntl(0, F_SETPIPE_SZ, 1 << 20); (void)fcntl(1, F_SETPIPE_SZ, 1 << 20);   /* the reference's pipelines: fewer wake-ups per megabyte (fails harmlessly on files) */
#endif
	if (!strcmp(argv[1], "sort")) ssg_worker_begin();
	inflate_hook_setup();
	if (!strcmp(argv[1], "view")) return cmd_view(argc - 2, argv + 2);
	if (!strcmp(argv[1], "sort")) { ssg_stamp("sambamba_sort", "start"); const int rc = cmd_sort(argc - 2, argv + 2); ssg_stamp("sambamba_sort", "end"); ssg_worker_done(rc); return ssg_fast_exit(rc); }
	if (!strcmp(argv[1], "index")) { ssg_stamp("sambamba_index", "start"); const int rc = cmd_index(argc - 2, argv + 2); ssg_stamp("sambamba_index", "end"); return rc; }
	if (!strcmp(argv[1], "flagstat")) return cmd_flagstat(argc - 2, argv + 2);
	if (!strcmp(argv[1], "merge")) return cmd_merge(argc - 2, argv + 2);
	if (!strcmp(argv[1], "depth")) return cmd_depth(argc - 2, argv + 2);
	if (!strcmp(argv[1], "stats")) return cmd_stats(argc - 2, argv + 2);
	if (!strcmp(argv[1], "markdup")) return cmd_markdup(argc - 2, argv + 2);
	if (!strcmp(argv[1], "index-parts")) return cmd_index_parts(argc - 2, argv + 2);
	fprintf(stderr, "[sambamba] unsupported sub-command %s\n", argv[1]);
	return 2;
}
