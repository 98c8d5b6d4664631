/*
 * ssg_stats.cpp -- ssg_stats_create / push / finish / get / free: the QC tables of `samtools stats' for records that lie in the record store (k_stats.h; the
 * program whose numbers it gives: samtools 1.3.1 stats.c).  A push scans a chunk with the scan's own host code (recs_scan_dev, ssg_bam_scan.cpp) and decides its
 * records on the device.  The deciding kernel adds to the small tables at once; a copy of them taken before the launch is put back when the kernel reports a
 * refusal, and the per-base, checksum and coverage kernels run only behind a decision without one: a failed push leaves the object as it was.  The coverage
 * window is kept as differences (as ssg_depth.cpp keeps a span) and slides with the stream: the tree's exclusive sum (ssg_prim.h) finishes it, a histogram
 * kernel adds its depths to the bins, and the slack's unfinished differences are carried into the next window, so no position is counted as two partial depths.
 * A translation unit of its own: the machine code of the pinned kernels does not move (tools/isa_pin.py).
 */
#include <algorithm>
#include <string>
#include <vector>
#include "ssg_rt.h"
#include "k_stats.h"
#include "ssg_prim.h"
#include "../../include/ssgpu.h"
#include "ssg_recs_int.h"

/* the options as samtools rounds them (init_stat_structs): the step no wider than the range, the maximum on the last bin's end */
static bool stats_opt_ok(const ssg_stats_opt_t *o, ssg_stats_opt_t &r, int64_t &n_cov, std::string &why)
{
	if (!o) { why = "no options"; return false; }
	r = *o;
	if (r.max_len < 1 || r.max_len > 65535) { why = "max_len outside 1 .. 65535"; return false; }
	if (r.n_isize < 1 || r.n_isize > (1 << 24)) { why = "n_isize outside 1 .. 2^24"; return false; }
	if (r.cov_min < 0 || r.cov_max < r.cov_min || r.cov_max > (1 << 24) || r.cov_step < 1) { why = "not 0 <= cov_min <= cov_max <= 2^24 and cov_step >= 1"; return false; }
	if (r.span < 0 || r.span > (1 << 28)) { why = "span outside 0 .. 2^28"; return false; }
	if (r.span == 0) r.span = 1 << 22;
	if (r.cov_step > r.cov_max - r.cov_min + 1) { r.cov_step = r.cov_max - r.cov_min; if (r.cov_step <= 0) r.cov_step = 1; }
	n_cov = 3 + (int64_t)(r.cov_max - r.cov_min) / r.cov_step;
	r.cov_max = r.cov_min + ((r.cov_max - r.cov_min) / r.cov_step + 1) * r.cov_step - 1;
	if (n_cov > STATS_COV_MAX) { why = "more than " + std::to_string(STATS_COV_MAX) + " coverage bins"; return false; }
	return true;
}

/* the tables: one allocation of 64-bit integers, the small ones (what the deciding kernel adds to) first */
struct ssg_stats {
	ssg_recs *r; std::vector<ssg_bam_fop_t> prog; ssg_bam_fop_t *d_prog; ssg_stats_opt_t o; int64_t n_cov; int32_t tile; int64_t slab;
	int state;   /* 0 takes pushes; 1 finished */
	unsigned long long *d_tab, *d_bak; size_t n_small, n_all, o_gc, o_isz, o_rl, o_id, o_ic, o_quals, o_bases, o_cov;
	bool sorted, have_last; uint64_t last_key;
	bool win_open; int64_t win_tid, win_beg, win_hi, n_arr; uint32_t *d_diff, *d_next, *d_ex;   /* the window: n_arr = span + max_len + 1 differences and one zero behind them; no record reaches position win_hi of it */
	ssg_stats() : r(0), d_prog(0), n_cov(0), tile(0), slab(0), state(0), d_tab(0), d_bak(0), n_small(0), n_all(0), sorted(true), have_last(false), last_key(0),
	              win_open(false), win_tid(0), win_beg(0), win_hi(0), n_arr(0), d_diff(0), d_next(0), d_ex(0) {}
	stats_tab_t tab() const
	{
		stats_tab_t t; t.sc = d_tab; t.gc = d_tab + o_gc; t.isz = d_tab + o_isz; t.rl = d_tab + o_rl; t.id = d_tab + o_id; t.ic = d_tab + o_ic;
		t.quals = d_tab + o_quals; t.bases = d_tab + o_bases; t.cov = d_tab + o_cov; t.rows = o.max_len + 1; t.n_isize = o.n_isize;
		return t;
	}
};
static int stats_usable(const ssg_stats *s, const char *who)
{
	if (rt_device_count() < 1) { ssg_err_msg = "no HIP device visible: libssgpu has no CPU path"; return SSG_ENODEV; }
	if (!s) { ssg_err_msg = std::string(who) + ": no object"; return SSG_EINVAL; }
	return recs_usable(s->r, who);
}
static void stats_win_drop(ssg_stats *s)
{
	rt_free(s->d_diff); rt_free(s->d_next); rt_free(s->d_ex);
	s->d_diff = s->d_next = s->d_ex = 0; s->win_open = false;
}
/* the depths of the window's first n positions into the bins (d_ex holds the sums of the first n + 2 differences behind this) */
static int stats_win_hist(ssg_stats *s, int64_t n)
{
	CHK((prim_exsum<uint32_t, uint32_t>(s->d_diff, s->d_ex, std::min<int64_t>(n + 2, s->n_arr + 1))));
	const uint64_t grid = std::min<uint64_t>(((uint64_t)n + 255) / 256, 1024);
	SSG_LAUNCH(ssg_k_stats_cov_hist, grid, 256, 0, (const uint32_t*)s->d_ex, n, s->o.cov_min, s->o.cov_max, s->o.cov_step, (int32_t)s->n_cov, s->d_tab + s->o_cov);
	return 0;
}
/* the window moves on by span positions */
static int stats_win_slide(ssg_stats *s)
{
	CHK(stats_win_hist(s, s->o.span));
	SSG_LAUNCH(ssg_k_stats_cov_carry, ((uint64_t)s->n_arr + 1 + 255) / 256, 256, 0, (const uint32_t*)s->d_ex, (const uint32_t*)s->d_diff, (int64_t)s->o.span, s->n_arr, s->d_next);
	std::swap(s->d_diff, s->d_next);
	s->win_beg += s->o.span; s->win_hi = std::max<int64_t>(s->win_hi - s->o.span, 0);
	return 0;
}
/* every position of the window is finished */
static int stats_win_flush(ssg_stats *s)
{
	if (!s->win_open) return 0;
	if (s->win_hi > 0) CHK(stats_win_hist(s, std::min(s->win_hi, s->n_arr)));   /* (behind win_hi every depth is 0) */
	s->win_open = false;
	return 0;
}
static int stats_win_open(ssg_stats *s, int64_t tid, int64_t beg)
{
	const size_t bytes = ((size_t)s->n_arr + 1) * 4;
	if (!s->d_diff) {
		s->d_diff = (uint32_t*)rt_malloc(bytes); s->d_next = (uint32_t*)rt_malloc(bytes); s->d_ex = (uint32_t*)rt_malloc(bytes);
		if (!s->d_diff || !s->d_next || !s->d_ex) { stats_win_drop(s); ssg_err_msg = "device allocation failed: the coverage window of " + std::to_string(s->n_arr) + " positions"; return SSG_ENOMEM; }
	}
	CHK(rt_memset(s->d_diff, 0, bytes));
	s->win_open = true; s->win_tid = tid; s->win_beg = beg; s->win_hi = 0;
	return 0;
}

extern "C" {

int64_t ssg_stats_ncov(const ssg_stats_opt_t *opt)
{
	ssg_stats_opt_t r; int64_t n = 0; std::string why;
	return stats_opt_ok(opt, r, n, why) ? n : -1;
}

int ssg_stats_create(ssg_recs_t *r, const ssg_bam_fop_t *prog, int n_prog, const ssg_stats_opt_t *opt, ssg_stats_t **out)
{
	if (rt_device_count() < 1) { ssg_err_msg = "no HIP device visible: libssgpu has no CPU path"; return SSG_ENODEV; }
	if (!r) { ssg_err_msg = "ssg_stats_create: no record store"; return SSG_EINVAL; }
	CHK(recs_usable(r, "ssg_stats_create"));
	if (!out) { ssg_err_msg = "ssg_stats_create: no place for the handle"; return SSG_EINVAL; }
	CHK(recs_prog_ok("ssg_stats_create: ", prog, n_prog));
	ssg_stats_opt_t o; int64_t n_cov = 0; std::string why;
	if (!stats_opt_ok(opt, o, n_cov, why)) { ssg_err_msg = "ssg_stats_create: " + why; return SSG_EINVAL; }
	ssg_stats *s = new ssg_stats();
	s->r = r; s->o = o; s->n_cov = n_cov; s->prog.assign(prog, prog + n_prog);
	/* SSG_STATS_TILE: the cycles of the per-base kernel's LDS tile; SSG_STATS_SLAB: the records a workgroup of it takes; the tables depend on neither */
	const char *const te = getenv("SSG_STATS_TILE"), *const se = getenv("SSG_STATS_SLAB");
	s->tile = te && *te ? atoi(te) : STATS_TILE_MAX; s->slab = se && *se ? atoll(se) : 4096;
	s->tile = std::max(1, std::min(s->tile, STATS_TILE_MAX)); s->slab = std::max<int64_t>(1, std::min<int64_t>(s->slab, (int64_t)1 << 31));
	const size_t rows = (size_t)o.max_len + 1;
	size_t at = SSG_ST_N;
	s->o_gc = at; at += 2 * SSG_STATS_NGC; s->o_isz = at; at += 3 * (size_t)o.n_isize; s->o_rl = at; at += rows; s->o_id = at; at += 2 * SSG_STATS_NINDEL; s->o_ic = at; at += 4 * rows;
	s->n_small = at;
	s->o_quals = at; at += 2 * rows * 256; s->o_bases = at; at += rows * 6; s->o_cov = at; at += (size_t)n_cov;
	s->n_all = at;
	s->n_arr = (int64_t)o.span + (int64_t)o.max_len + 1;
	s->d_tab = (unsigned long long*)rt_malloc_raw(s->n_all * 8); s->d_bak = (unsigned long long*)rt_malloc_raw(s->n_small * 8);
	s->d_prog = (ssg_bam_fop_t*)rt_malloc_raw(((size_t)n_prog + 1) * sizeof(ssg_bam_fop_t));
	int rc = s->d_tab && s->d_bak && s->d_prog ? 0 : SSG_ENOMEM;
	if (rc) ssg_err_msg = "device allocation failed: the tables of ssg_stats_create";
	if (!rc) rc = rt_memset(s->d_tab, 0, s->n_all * 8);
	if (!rc && n_prog) rc = rt_h2d(s->d_prog, prog, (size_t)n_prog * sizeof(ssg_bam_fop_t));
	if (!rc) rc = rt_sync();
	if (rc) { rt_free_raw(s->d_tab); rt_free_raw(s->d_bak); rt_free_raw(s->d_prog); delete s; return rc; }
	*out = s;
	return 0;
}

void ssg_stats_free(ssg_stats_t *s)
{
	if (!s) return;
	(void)rt_sync();
	stats_win_drop(s);
	rt_free_raw(s->d_tab); rt_free_raw(s->d_bak); rt_free_raw(s->d_prog);
	delete s;
}

int ssg_stats_push(ssg_stats_t *s, uint32_t chunk_id, const uint64_t *hint, int64_t n_hints, uint64_t first, uint64_t *n_rec, uint64_t *descents)
{
	const std::string who = "ssg_stats_push";
	CHK(stats_usable(s, "ssg_stats_push"));
	if (!n_rec || !descents) { ssg_err_msg = who + ": no place for the numbers of records"; return SSG_EINVAL; }
	*n_rec = *descents = 0;
	if (s->state != 0) { ssg_err_msg = who + ": the object is finished (ssg_stats_finish was called)"; return SSG_EINVAL; }
	ssg_recs *const r = s->r;
	if (r->ordered) { ssg_err_msg = who + ": refused while an order is declared: ssg_recs_reopen first"; return SSG_EINVAL; }
	recs_scan_dev_t sc;
	CHK(recs_scan_dev(r, "ssg_stats_push", chunk_id, hint, n_hints, first, ~(uint64_t)0, true, n_rec, sc));
	const uint64_t n = *n_rec;
	if (n == 0) return 0;
	const uint64_t grid = (n + 255) / 256;   /* (below 2^31: the scan has checked it) */
	dbuf<uint8_t> d_cls((size_t)n), d_use((size_t)n); dbuf<uint32_t> d_idx((size_t)n), d_kept((size_t)n); dbuf<stats_pb_t> d_pb((size_t)n); dbuf<unsigned long long> d_err(STATS_ERR_N);
	if (!d_cls.ok() || !d_use.ok() || !d_idx.ok() || !d_kept.ok() || !d_pb.ok() || !d_err.ok()) { ssg_err_msg = "device allocation failed: the decisions of ssg_stats_push"; return SSG_ENOMEM; }
	CHK(rt_memset(d_err.p, 0, STATS_ERR_N * 8)); CHK(rt_memset(d_err.p, 0xff, STATS_PUSH_MAX * 8));
	CHK(rt_d2d(s->d_bak, s->d_tab, s->n_small * 8));
	const uint8_t *const d_chunk = r->d_chunk[chunk_id];
	const stats_tab_t T = s->tab();
	SSG_LAUNCH(ssg_k_stats_decide, grid, 256, 0, d_chunk, (const uint64_t*)sc.loc.p, (int64_t)n, (const ssg_bam_fop_t*)s->d_prog, (int32_t)s->prog.size(), T, d_cls.p, d_pb.p, d_use.p, d_idx.p, d_err.p);
	CHK(rt_sync());
	unsigned long long err[STATS_ERR_N]; CHK(d_err.down(err, STATS_ERR_N));
	int refused = 0;
	if (err[STATS_ERR_FIT] != ~0ull) { refused = SSG_EIO; ssg_err_msg = who + ": malformed record at offset " + std::to_string(err[STATS_ERR_FIT]) + ": 32 + l_qname + 4 n_cigar + (l_seq + 1) / 2 + l_seq exceeds block_size"; }
	else if (err[STATS_ERR_LONG] != ~0ull) { refused = SSG_ERANGE; ssg_err_msg = who + ": the record at offset " + std::to_string(err[STATS_ERR_LONG]) + " has an unclipped length above max_len = " + std::to_string(s->o.max_len); }
	else if (err[STATS_ERR_NOCIGAR] != ~0ull) { refused = SSG_EIO; ssg_err_msg = who + ": the record at offset " + std::to_string(err[STATS_ERR_NOCIGAR]) + " is mapped and has no CIGAR"; }
	else if (err[STATS_ERR_CYCLE] != ~0ull) { refused = SSG_EIO; ssg_err_msg = who + ": the CIGAR of the record at offset " + std::to_string(err[STATS_ERR_CYCLE]) + " puts an insertion or deletion outside the cycles 0 .. " + std::to_string(s->o.max_len); }
	if (refused) {
		const std::string msg = ssg_err_msg;
		CHK(rt_d2d(s->d_tab, s->d_bak, s->n_small * 8)); CHK(rt_sync());
		ssg_err_msg = msg;
		return refused;
	}
	/* decided without a refusal: the checksums, the bases, the coverage */
	SSG_LAUNCH(ssg_k_stats_crc, grid, 256, 0, d_chunk, (const uint64_t*)sc.loc.p, (const uint8_t*)d_cls.p, (int64_t)n, s->d_tab);
	const int64_t longest = (int64_t)err[STATS_PUSH_MAX];
	if (longest > 0) {
		const int64_t n_tiles = (longest + s->tile - 1) / s->tile;
		int64_t slab = s->slab;
		while (n_tiles * (((int64_t)n + slab - 1) / slab) > 0x7fffffffll) slab *= 2;   /* (a launch stays below 2^31 workgroups) */
		SSG_LAUNCH(ssg_k_stats_bases, (uint64_t)(n_tiles * (((int64_t)n + slab - 1) / slab)), 256, 0, d_chunk, (const stats_pb_t*)d_pb.p, (int64_t)n, s->tile, slab, (int32_t)n_tiles, T);
	}
	if (s->sorted) {
		uint64_t m = 0;
		CHK(prim_select((const uint32_t*)d_idx.p, (const uint8_t*)d_use.p, (int64_t)n, d_kept.p, &m));
		if (m > n) { ssg_err_msg = who + ": the selection returned " + std::to_string(m) + " of " + std::to_string(n) + " records"; return SSG_EHIP; }
		if (m > 0) {
			dbuf<uint64_t> d_ckey((size_t)m); dbuf<unsigned long long> d_cnt(1);
			if (!d_ckey.ok() || !d_cnt.ok()) { ssg_err_msg = "device allocation failed: the keys of ssg_stats_push"; return SSG_ENOMEM; }
			CHK(d_cnt.zero());
			SSG_LAUNCH(ssg_k_stats_ckeys, (m + 255) / 256, 256, 0, d_chunk, (const uint64_t*)sc.loc.p, (const uint32_t*)d_kept.p, (int64_t)m, s->last_key, (int32_t)(s->have_last ? 1 : 0), d_ckey.p, d_cnt.p);
			CHK(rt_sync());
			unsigned long long desc = 0; CHK(d_cnt.down(&desc, 1));
			std::vector<uint64_t> ckey((size_t)m); CHK(d_ckey.down(ckey.data(), (size_t)m));
			*descents = desc;
			if (desc) {   /* coverage is off for good */
				s->sorted = false; stats_win_drop(s);
				CHK(rt_memset(s->d_tab + s->o_cov, 0, (size_t)s->n_cov * 8));
			} else {
				const int64_t span = s->o.span, slack = s->o.max_len;
				size_t c = 0;
				while (c < (size_t)m) {
					const int64_t tid = (int64_t)(ckey[c] >> 32), pos = (int64_t)(ckey[c] & 0xffffffffu);
					if (s->win_open && (tid != s->win_tid || pos >= s->win_beg + span + slack)) CHK(stats_win_flush(s));   /* a new contig or a far jump: the tail is finished too */
					if (!s->win_open) CHK(stats_win_open(s, tid, pos));
					while (pos >= s->win_beg + span) CHK(stats_win_slide(s));
					const int64_t top = s->win_beg + span;   /* the records that begin inside the window */
					const size_t e = top > 0xffffffffll ? (size_t)(std::upper_bound(ckey.begin() + (ptrdiff_t)c, ckey.end(), (uint64_t)tid << 32 | 0xffffffffu) - ckey.begin())
					                                     : (size_t)(std::lower_bound(ckey.begin() + (ptrdiff_t)c, ckey.end(), (uint64_t)tid << 32 | (uint64_t)top) - ckey.begin());
					SSG_LAUNCH(ssg_k_stats_cov_add, ((uint64_t)(e - c) + 255) / 256, 256, 0, d_chunk, (const uint64_t*)sc.loc.p, (const uint32_t*)d_kept.p, (int64_t)c, (int64_t)e, s->win_beg, s->n_arr, s->d_diff);
					if (e > c) s->win_hi = std::max<int64_t>(s->win_hi, (int64_t)(ckey[e - 1] & 0xffffffffu) - s->win_beg + slack + 1);
					c = e;
				}
			}
			s->last_key = ckey[(size_t)m - 1]; s->have_last = true;
		}
	}
	return rt_sync();
}

int ssg_stats_finish(ssg_stats_t *s)
{
	CHK(stats_usable(s, "ssg_stats_finish"));
	if (s->state != 0) { ssg_err_msg = "ssg_stats_finish: the object is finished already"; return SSG_EINVAL; }
	if (s->sorted) CHK(stats_win_flush(s));
	CHK(rt_sync());
	stats_win_drop(s);
	s->state = 1;
	return 0;
}

int ssg_stats_get(ssg_stats_t *s, uint64_t *scalars, uint64_t *quals, uint64_t *bases, uint64_t *gc, uint64_t *isize, uint64_t *rl, uint64_t *id, uint64_t *ic, uint64_t *cov)
{
	CHK(stats_usable(s, "ssg_stats_get"));
	CHK(rt_sync());
	static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit tables");
	const size_t rows = (size_t)s->o.max_len + 1;
	std::vector<uint64_t> small(s->n_small);
	CHK(rt_d2h(small.data(), s->d_tab, s->n_small * 8));
	if (scalars) {
		std::copy(small.begin(), small.begin() + SSG_ST_N, scalars);
		for (int k = SSG_ST_CHK_NAMES; k <= SSG_ST_CHK_QUALS; ++k) scalars[k] &= 0xffffffffu;   /* the sums wrap at 32 bits */
		scalars[SSG_ST_SORTED] = s->sorted ? 1 : 0;
	}
	if (gc) for (int f = 0; f < 2; ++f) { uint64_t t = 0; for (int k = 0; k < SSG_STATS_NGC; ++k) { t += small[s->o_gc + (size_t)f * SSG_STATS_NGC + (size_t)k]; gc[f * SSG_STATS_NGC + k] = t; } }
	if (isize) for (size_t k = 0; k < 3 * (size_t)s->o.n_isize; ++k) isize[k] = small[s->o_isz + k] / 2;
	if (rl) std::copy(small.begin() + (ptrdiff_t)s->o_rl, small.begin() + (ptrdiff_t)(s->o_rl + rows), rl);
	if (id) std::copy(small.begin() + (ptrdiff_t)s->o_id, small.begin() + (ptrdiff_t)(s->o_id + 2 * SSG_STATS_NINDEL), id);
	if (ic) std::copy(small.begin() + (ptrdiff_t)s->o_ic, small.begin() + (ptrdiff_t)(s->o_ic + 4 * rows), ic);
	if (quals) CHK(rt_d2h(quals, s->d_tab + s->o_quals, 2 * rows * 256 * 8));
	if (bases) CHK(rt_d2h(bases, s->d_tab + s->o_bases, rows * 6 * 8));
	if (cov) CHK(rt_d2h(cov, s->d_tab + s->o_cov, (size_t)s->n_cov * 8));
	return 0;
}

} /* extern "C" */
