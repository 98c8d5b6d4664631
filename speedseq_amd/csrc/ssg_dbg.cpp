/*
 * ssg_dbg.cpp -- the stage test entries of include/ssgpu.h: ssg_dbg_chain, ssg_dbg_regions, ssg_dbg_reg2aln, ssg_dbg_pestat, ssg_dbg_pair_final,
 * ssg_dbg_matesw, ssg_dbg_sbl_records, ssg_dbg_extend_coop and ssg_dbg_smem_ext.  Each checks lists built by the caller until nothing out of range can reach a kernel, lays them out as the stage before leaves them, and
 * runs the pipeline's own stage function on them (ssgpu_core.cpp, through ssg_stage_int.h).  A translation unit of its own so that the stage code of the core
 * reads without them -- and one that must never include a kernel header (k_*.h) or launch a kernel: the machine code of every kernel depends on what else
 * its unit holds, and that code is pinned (tools/isa_pin.py).  Device work goes through dbuf<> and the core's host functions.
 * Every refusal is SSG_EINVAL with a message "<entry>: <what> <index>"; tests/test_dbg_refusals.py holds the messages and the order of the checks.
 */
#include <vector>
#include <string>
#include <algorithm>
#include "ssg_rt.h"
#include "../../include/ssgpu.h"
#include "ssg_index_int.h"
#include "ssg_pe_int.h"
#include "ssg_stage_int.h"

SSG_ABI_FP_DEFINE(dbg)

/* ---- what the entries share ---- */
static int dbg_refuse(const char *who, const char *bad, long at)
{
	ssg_err_msg = std::string(who) + ": " + bad + " " + std::to_string(at);
	return SSG_EINVAL;
}
static int dbg_check_contigs(const char *who, int64_t l_pac, int n_ctg, const int64_t *ctg_off, const int32_t *ctg_len)
{
	for (int c = 0; c < n_ctg; ++c)
		if (ctg_len[c] < 1 || ctg_off[c] != (c ? ctg_off[c - 1] + ctg_len[c - 1] : 0) || ctg_off[c] + ctg_len[c] > l_pac || (c == n_ctg - 1 && ctg_off[c] + ctg_len[c] != l_pac)) {
			ssg_err_msg = std::string(who) + ": the contigs must tile [0, l_pac) in order"; return SSG_EINVAL; }
	return 0;
}
/* The reads, one at a time (ssg_dbg_regions checks a read's seeds and chains before the next read's offsets): off must not decrease at read r and the length is
 * 1 .. SSG_MAX_READ_LEN, then the codes are 0 .. 4.  Each sets *bad where it objects; dbg_read_len returns the length.  (That off starts at 0 is the caller's:
 * one message covers all its offset arrays.  ssg_dbg_matesw words its read checks differently and keeps them.) */
static int dbg_read_len(const int64_t *off, int r, const char **bad)
{
	const int64_t len = off[r + 1] - off[r];
	if (len < 0) *bad = "offsets must not decrease: read";
	else if (len < 1 || len > SSG_MAX_READ_LEN) *bad = "need 1 <= read length <= " SSG_STR(SSG_MAX_READ_LEN) ": read";
	return *bad ? 0 : (int)len;
}
static void dbg_check_codes(const uint8_t *seq, const int64_t *off, int r, const char **bad)
{
	for (int64_t k = off[r]; k < off[r + 1]; ++k) if (seq[k] > 4) { *bad = "read codes are 0 .. 4: read"; return; }
}
/* a seed's geometry against its read of len bases and the doubled reference: 0, or what is wrong (outside_read: the entry's words for the first check) */
static const char *dbg_check_seed(const ssg_seed_t &s, int len, int64_t l_pac, const char *outside_read)
{
	if (!(0 <= s.qbeg && 1 <= s.len && s.qbeg <= len - s.len)) return outside_read;
	if (!(0 <= s.rbeg && s.rbeg <= 2 * l_pac - s.len)) return "need 0 <= rbeg, rbeg + len <= 2 l_pac: seed";
	return 0;
}
/* a reference given by the caller, in HBM: the view has pac, l_pac and the contig table and nothing else of an index */
struct dbg_ref_t {
	dbuf<uint8_t> d_pac; dbuf<int64_t> d_coff; dbuf<int32_t> d_clen; ssg_index_view_t ix;
	int up(const uint8_t *pac, int64_t l_pac, int n_ctg, const int64_t *ctg_off, const int32_t *ctg_len)
	{
		const size_t pac_bytes = (size_t)(l_pac / 4 + 1);
		d_pac.alloc(pac_bytes); d_coff.alloc((size_t)n_ctg); d_clen.alloc((size_t)n_ctg);
		CHKA(d_pac); CHKA(d_coff); CHKA(d_clen);
		CHK(d_pac.up(pac, pac_bytes)); CHK(d_coff.up(ctg_off, (size_t)n_ctg)); CHK(d_clen.up(ctg_len, (size_t)n_ctg));
		memset(&ix, 0, sizeof(ix));
		ix.pac = d_pac.p; ix.ctg_off = d_coff.p; ix.ctg_len = d_clen.p; ix.l_pac = l_pac; ix.n_ctg = n_ctg;
		return 0;
	}
};
/* seeds as the seeding stage leaves them: score = len, no link; tot + 1 entries, the last one zero */
static std::vector<ssg_seed_t> dbg_stage_seeds(const ssg_seed_t *seeds, int64_t tot)
{
	std::vector<ssg_seed_t> h((size_t)tot + 1);
	memset(h.data(), 0, h.size() * sizeof(ssg_seed_t));
	for (int64_t k = 0; k < tot; ++k) { h[k] = seeds[k]; h[k].score = seeds[k].len; h[k].next = -1; }
	return h;
}
/* per-read counts of an offset array */
static std::vector<int32_t> dbg_counts(const int64_t *off, int n)
{
	std::vector<int32_t> c((size_t)n);
	for (int r = 0; r < n; ++r) c[r] = (int32_t)(off[r + 1] - off[r]);
	return c;
}
/* the work order as run_align1 makes it: the reads heaviest first by d_key, and zeroed queue counters */
static int dbg_work_order(const int32_t *d_key, int n_reads, int32_t *d_work, dbuf<unsigned int> &d_queue)
{
	CHK(dev_order_desc(d_key, d_work, n_reads)); CHK(rt_sync());
	return d_queue.zero();
}

/* test entry: the chaining stage on the caller's seeds and intervals (include/ssgpu.h), through run_chain as stage 1 goes through it */
int ssg_dbg_chain(const ssg_mem_opt_t *opt, int64_t l_pac, int n_ctg, int n_reads, const int32_t *read_len, const int64_t *seed_off, const ssg_seed_t *seeds, const int32_t *rids,
                  const int64_t *intv_off, const ssg_intv_t *intv, int64_t *chain_off, ssg_chain_t **chains, int32_t **chain_seeds, int32_t *form)
{
	CHK(ssg_need_device());
	*chains = 0; *chain_seeds = 0;
	if (n_reads < 0 || l_pac < 1 || l_pac >= (int64_t)1 << 33 || n_ctg < 1) { ssg_err_msg = "ssg_dbg_chain: need n_reads >= 0, 1 <= l_pac < 2^33, n_ctg >= 1"; return SSG_EINVAL; }
	if (n_reads == 0) { chain_off[0] = 0; return SSG_OK; }
	const char *bad = 0; long at = 0;
	if (seed_off[0] != 0 || intv_off[0] != 0) bad = "offsets start at 0: read";
	int max_len = 0, cap = 1;
	for (int r = 0; !bad && r < n_reads; ++r) {
		const int len = read_len[r];
		at = r;
		if (seed_off[r + 1] < seed_off[r] || intv_off[r + 1] < intv_off[r]) { bad = "offsets must not decrease: read"; break; }
		if (seed_off[r + 1] - seed_off[r] >= (int64_t)1 << 24 || intv_off[r + 1] - intv_off[r] >= (int64_t)1 << 24) { bad = "more than 2^24 seeds or intervals: read"; break; }
		if (len < 1 || len > SSG_MAX_READ_LEN) { bad = "need 1 <= read_len <= " SSG_STR(SSG_MAX_READ_LEN) ": read"; break; }
		max_len = std::max(max_len, len); cap = std::max(cap, (int)(intv_off[r + 1] - intv_off[r]));
		for (int64_t k = seed_off[r]; !bad && k < seed_off[r + 1]; ++k) {
			bad = dbg_check_seed(seeds[k], len, l_pac, "need 0 <= qbeg, 1 <= len, qbeg + len <= read_len: seed");
			if (!bad && rids[k] >= n_ctg) bad = "rid beyond the contigs: seed";
			if (bad) at = (long)k;
		}
		int64_t prev = 0;
		for (int64_t k = intv_off[r]; !bad && k < intv_off[r + 1]; ++k) {
			const int64_t sb = (int64_t)(intv[k].info >> 32), se = (int64_t)(uint32_t)intv[k].info;
			if (!(sb < se && se <= len)) bad = "need 0 <= start < end <= read_len: interval";
			else if (sb < prev) bad = "intervals must be sorted by start: interval";
			prev = sb;
			if (bad) at = (long)k;
		}
	}
	if (bad) return dbg_refuse("ssg_dbg_chain", bad, at);
	const int64_t tot = seed_off[n_reads];
	if (tot >= (int64_t)1 << 31) { ssg_err_msg = "ssg_dbg_chain: more than 2^31 seeds"; return SSG_EINVAL; }
	/* the stage's inputs as the seeding stage leaves them: read offsets, the dense interval layout (cap entries a read), seeds with score = len */
	const size_t ts = (size_t)tot + 1;
	std::vector<int64_t> h_off((size_t)n_reads + 1, 0);
	const std::vector<int32_t> h_ni = dbg_counts(intv_off, n_reads), h_ns = dbg_counts(seed_off, n_reads);
	std::vector<ssg_intv_t> h_iv((size_t)n_reads * cap);
	const std::vector<ssg_seed_t> h_sd = dbg_stage_seeds(seeds, tot);
	memset(h_iv.data(), 0, h_iv.size() * sizeof(ssg_intv_t));
	for (int r = 0; r < n_reads; ++r) {
		h_off[r + 1] = h_off[r] + read_len[r];
		for (int k = 0; k < h_ni[r]; ++k) h_iv[(size_t)r * cap + k] = intv[intv_off[r] + k];
	}
	ssg_index_view_t ix; memset(&ix, 0, sizeof(ix));
	ix.l_pac = l_pac; ix.n_ctg = n_ctg;
	dbuf<int64_t> d_off((size_t)n_reads + 1), d_soff((size_t)n_reads + 1); dbuf<ssg_intv_t> d_intv((size_t)n_reads * cap); dbuf<int32_t> d_nintv(n_reads), d_nseed(n_reads);
	dbuf<ssg_seed_t> d_seeds(ts); dbuf<int32_t> d_srid(ts), d_order(ts), d_kept(ts), d_cseeds(ts), d_nchain(n_reads), d_work(n_reads); dbuf<ssg_chain_t> d_chains(ts); dbuf<unsigned int> d_queue(8);
	CHKA(d_off); CHKA(d_soff); CHKA(d_intv); CHKA(d_nintv); CHKA(d_nseed); CHKA(d_seeds); CHKA(d_srid); CHKA(d_order); CHKA(d_kept); CHKA(d_cseeds); CHKA(d_nchain); CHKA(d_work); CHKA(d_chains); CHKA(d_queue);
	CHK(d_off.up(h_off.data(), (size_t)n_reads + 1)); CHK(d_soff.up(seed_off, (size_t)n_reads + 1)); CHK(d_intv.up(h_iv.data(), h_iv.size())); CHK(d_nintv.up(h_ni.data(), n_reads));
	CHK(d_nseed.up(h_ns.data(), n_reads)); CHK(d_seeds.up(h_sd.data(), (size_t)tot)); CHK(d_srid.up(rids, (size_t)tot)); CHK(d_nchain.zero());
	CHK(dbg_work_order(d_nseed.p, n_reads, d_work.p, d_queue));
	CHK(run_chain(ix, opt, n_reads, d_off.p, max_len, d_intv.p, d_nintv.p, cap, d_nseed.p, d_soff.p, d_seeds.p, d_srid.p, d_chains.p, d_order.p, d_kept.p, d_cseeds.p, d_nchain.p,
	              d_work.p, d_queue.p, (uint64_t*)0, form));
	CHK(rt_sync());
	std::vector<int32_t> h_nc((size_t)n_reads), h_ord(ts), h_cs(ts); std::vector<ssg_chain_t> h_ch(ts);
	CHK(d_nchain.down(h_nc.data(), n_reads)); CHK(d_order.down(h_ord.data(), (size_t)tot)); CHK(d_cseeds.down(h_cs.data(), (size_t)tot)); CHK(d_chains.down(h_ch.data(), (size_t)tot));
	/* the survivors in the stage's order; what the kernels left is checked against the slices before it is followed */
	int64_t n_out = 0, n_sd = 0;
	for (int r = 0; r < n_reads; ++r) {
		if (h_nc[r] < 0 || h_nc[r] > h_ns[r]) { ssg_err_msg = "ssg_dbg_chain: a read's chain count is outside its slice"; return SSG_EOVERFLOW; }
		for (int i = 0; i < h_nc[r]; ++i) {
			const int32_t id = h_ord[seed_off[r] + i];
			if (id < 0 || id >= h_ns[r]) { ssg_err_msg = "ssg_dbg_chain: a chain id is outside its read's slice"; return SSG_EOVERFLOW; }
			const ssg_chain_t &c = h_ch[seed_off[r] + id];
			if (c.n < 1 || c.first_seed < seed_off[r] || (int64_t)c.first_seed + c.n > seed_off[r + 1]) { ssg_err_msg = "ssg_dbg_chain: a chain's seed list is outside its read's slice"; return SSG_EOVERFLOW; }
			++n_out; n_sd += c.n;
		}
	}
	ssg_chain_t *oc = (ssg_chain_t*)calloc((size_t)n_out + 1, sizeof(ssg_chain_t)); int32_t *os = (int32_t*)calloc((size_t)n_sd + 1, sizeof(int32_t));
	if (!oc || !os) { free(oc); free(os); ssg_err_msg = "host allocation failed: chains"; return SSG_ENOMEM; }
	int64_t k = 0, q = 0;
	for (int r = 0; r < n_reads; ++r) {
		chain_off[r] = k;
		for (int i = 0; i < h_nc[r]; ++i) {
			const ssg_chain_t &c = h_ch[seed_off[r] + h_ord[seed_off[r] + i]];
			ssg_chain_t &o = oc[k++];
			o.pos = c.pos; o.rid = c.rid; o.n = c.n; o.w = c.w; o.kept = c.kept; o.frac_rep = c.frac_rep; o.first_seed = (int32_t)q;
			for (int j = 0; j < c.n; ++j) os[q++] = (int32_t)(h_cs[c.first_seed + j] - seed_off[r]);
		}
	}
	chain_off[n_reads] = k;
	*chains = oc; *chain_seeds = os;
	return SSG_OK;
}

/* test entry: the region stage on the caller's chains (include/ssgpu.h), through run_regions as stage 1 goes through it */
int ssg_dbg_regions(const ssg_mem_opt_t *opt, const uint8_t *pac, int64_t l_pac, int n_ctg, const int64_t *ctg_off, const int32_t *ctg_len, int n_reads, const uint8_t *seq, const int64_t *off,
                    const int64_t *seed_off, const ssg_seed_t *seeds, const int64_t *chain_off, const ssg_chain_t *chains, const int32_t *chain_seeds,
                    int64_t *reg_off, ssg_alnreg_t **regs, int32_t *route)
{
	CHK(ssg_need_device());
	*regs = 0;
	if (n_reads < 0 || l_pac < 1 || l_pac >= (int64_t)1 << 33 || n_ctg < 1) { ssg_err_msg = "ssg_dbg_regions: need n_reads >= 0, 1 <= l_pac < 2^33, n_ctg >= 1"; return SSG_EINVAL; }
	CHK(dbg_check_contigs("ssg_dbg_regions", l_pac, n_ctg, ctg_off, ctg_len));
	if (n_reads == 0) { reg_off[0] = 0; return SSG_OK; }
	const char *bad = 0; long at = 0;
	if (off[0] != 0 || seed_off[0] != 0 || chain_off[0] != 0) bad = "offsets start at 0: read";
	int max_len = 0;
	auto ctg_of = [&](int64_t p) { const int64_t f = p < l_pac ? p : 2 * l_pac - 1 - p; int lo = 0, hi = n_ctg - 1; while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (ctg_off[mid] <= f) lo = mid; else hi = mid - 1; } return lo; };
	std::vector<uint8_t> used;
	for (int r = 0; !bad && r < n_reads; ++r) {
		at = r;
		if (seed_off[r + 1] < seed_off[r] || chain_off[r + 1] < chain_off[r]) { bad = "offsets must not decrease: read"; break; }
		const int len = dbg_read_len(off, r, &bad);
		if (bad) break;
		const int64_t ns = seed_off[r + 1] - seed_off[r], nc = chain_off[r + 1] - chain_off[r];
		if (ns >= (int64_t)1 << 24) { bad = "more than 2^24 seeds: read"; break; }
		if (nc > ns) { bad = "more chains than seeds: read"; break; }
		max_len = std::max(max_len, len);
		dbg_check_codes(seq, off, r, &bad);
		for (int64_t k = seed_off[r]; !bad && k < seed_off[r + 1]; ++k) {
			bad = dbg_check_seed(seeds[k], len, l_pac, "need 0 <= qbeg, 1 <= len, qbeg + len <= read length: seed");
			if (bad) at = (long)k;
		}
		used.assign((size_t)ns, 0);
		for (int64_t k = chain_off[r]; !bad && k < chain_off[r + 1]; ++k) {
			const ssg_chain_t &c = chains[k];
			at = (long)k;
			if (c.n < 1) { bad = "a chain has at least 1 seed: chain"; break; }
			if (c.first_seed < 0 || (k > 0 && c.first_seed != chains[k - 1].first_seed + chains[k - 1].n) || (k == 0 && c.first_seed != 0)) { bad = "first_seed must run on from the chain before: chain"; break; }
			for (int j = 0; j < c.n; ++j) {
				const int32_t id = chain_seeds[c.first_seed + j];
				if (id < 0 || id >= ns) { bad = "a seed index outside the read's seeds: chain"; break; }
				if (used[(size_t)id]) { bad = "a seed in two chains: chain"; break; }
				used[(size_t)id] = 1;
			}
			if (bad) break;
			const int64_t first = seeds[seed_off[r] + chain_seeds[c.first_seed]].rbeg;
			if (c.rid != ctg_of(first)) { bad = "rid must be the contig of the chain's first seed: chain"; break; }
			/* the window is cut to the first seed's contig and strand (ssg_k_ext_prep): a seed outside it would index the window out of range */
			int64_t cb = ctg_off[c.rid], ce = cb + ctg_len[c.rid];
			if (first >= l_pac) { const int64_t t = cb; cb = 2 * l_pac - ce; ce = 2 * l_pac - t; }
			for (int j = 0; j < c.n; ++j) {
				const ssg_seed_t &sd = seeds[seed_off[r] + chain_seeds[c.first_seed + j]];
				if (sd.rbeg < cb || sd.rbeg + sd.len > ce) { bad = "every seed of a chain must lie inside the contig and strand of its first seed: chain"; break; }
			}
			if (bad) break;
		}
	}
	if (!bad) {   /* the scoring limits of the pipeline, whatever the chains: run_regions checks them only where there is a job */
		CHK(check_scores(opt, max_len));
		if (opt->e_del < 1 || opt->e_ins < 1) { ssg_err_msg = "ssg_dbg_regions: gap extension penalties must be positive"; return SSG_EINVAL; }
	}
	if (bad) return dbg_refuse("ssg_dbg_regions", bad, at);
	const int64_t tot = seed_off[n_reads];
	if (tot >= (int64_t)1 << 31) { ssg_err_msg = "ssg_dbg_regions: more than 2^31 seeds"; return SSG_EINVAL; }
	/* the stage's inputs as the chaining stage leaves them: per read a slice at seed_off[r] of chain records, their order and their seed lists (absolute indices) */
	const size_t ts = (size_t)tot + 1;
	const std::vector<ssg_seed_t> h_sd = dbg_stage_seeds(seeds, tot);
	std::vector<ssg_chain_t> h_ch(ts); std::vector<int32_t> h_ord(ts, 0), h_cs(ts, 0);
	const std::vector<int32_t> h_nc = dbg_counts(chain_off, n_reads), h_ns = dbg_counts(seed_off, n_reads);
	memset(h_ch.data(), 0, ts * sizeof(ssg_chain_t));
	for (int r = 0; r < n_reads; ++r) {
		const int64_t s0 = seed_off[r];
		int64_t q = s0;
		for (int i = 0; i < h_nc[r]; ++i) {
			const ssg_chain_t &c = chains[chain_off[r] + i];
			ssg_chain_t &d = h_ch[s0 + i];
			d = c; d.first_seed = (int32_t)q; d.last_seed = -1;
			h_ord[s0 + i] = i;
			for (int j = 0; j < c.n; ++j) h_cs[q++] = (int32_t)(s0 + chain_seeds[c.first_seed + j]);
		}
	}
	dbg_ref_t ref;
	CHK(ref.up(pac, l_pac, n_ctg, ctg_off, ctg_len));
	dbuf<uint8_t> d_seq((size_t)off[n_reads] + 1); dbuf<int64_t> d_off((size_t)n_reads + 1);
	dbuf<ssg_seed_t> d_seeds(ts); dbuf<ssg_chain_t> d_chains(ts); dbuf<int32_t> d_order(ts), d_cseeds(ts), d_nchain(n_reads), d_nseed(n_reads), d_work(n_reads); dbuf<unsigned int> d_queue(8);
	CHKA(d_seq); CHKA(d_off); CHKA(d_seeds); CHKA(d_chains); CHKA(d_order); CHKA(d_cseeds); CHKA(d_nchain); CHKA(d_nseed); CHKA(d_work); CHKA(d_queue);
	CHK(d_seq.up(seq, (size_t)off[n_reads])); CHK(d_off.up(off, (size_t)n_reads + 1));
	CHK(d_seeds.up(h_sd.data(), ts)); CHK(d_chains.up(h_ch.data(), ts)); CHK(d_order.up(h_ord.data(), ts)); CHK(d_cseeds.up(h_cs.data(), ts));
	CHK(d_nchain.up(h_nc.data(), n_reads)); CHK(d_nseed.up(h_ns.data(), n_reads));
	CHK(dbg_work_order(d_nseed.p, n_reads, d_work.p, d_queue));
	align1_dev_t o;
	if (!o.seed_off.alloc((size_t)n_reads + 1) || !o.regs.alloc(ts) || !o.n_reg.alloc(n_reads)) { ssg_err_msg = "device allocation failed: regs"; return SSG_ENOMEM; }
	CHK(o.seed_off.up(seed_off, (size_t)n_reads + 1));
	std::vector<int32_t> todo;
	CHK(run_regions(ref.ix, opt, n_reads, d_seq.p, d_off.p, max_len, ts, d_seeds.p, d_chains.p, d_order.p, d_cseeds.p, d_nchain.p, d_work.p, d_queue.p, o, (uint64_t*)0, (uint64_t*)0, &todo));
	std::vector<int32_t> hn((size_t)n_reads); std::vector<uint8_t> hf((size_t)n_reads); std::vector<ssg_alnreg_t> all(ts);
	CHK(o.n_reg.down(hn.data(), n_reads)); CHK(o.sdp_fixed.down(hf.data(), n_reads)); CHK(o.regs.down(all.data(), (size_t)tot));
	int64_t n_out = 0;
	for (int r = 0; r < n_reads; ++r) {
		if (hn[r] < 0 || hn[r] > h_ns[r]) { ssg_err_msg = "ssg_dbg_regions: a read's region count is outside its slice"; return SSG_EOVERFLOW; }
		reg_off[r] = n_out; n_out += hn[r];
	}
	reg_off[n_reads] = n_out;
	ssg_alnreg_t *out = (ssg_alnreg_t*)malloc(sizeof(ssg_alnreg_t) * (size_t)(n_out + 1));
	if (!out) { ssg_err_msg = "host allocation failed: regions"; return SSG_ENOMEM; }
	for (int r = 0; r < n_reads; ++r) memcpy(out + reg_off[r], all.data() + seed_off[r], sizeof(ssg_alnreg_t) * (size_t)hn[r]);
	if (route) {
		for (int r = 0; r < n_reads; ++r) route[r] = hf[r] == 0 ? SSG_REG_ROUTE_PATCH : 0;
		for (size_t k = 0; k < todo.size(); ++k) if (todo[k] >= 0 && todo[k] < n_reads) route[todo[k]] |= SSG_REG_ROUTE_WAVE;
	}
	*regs = out;
	return SSG_OK;
}

/* test entry: CIGAR / POS / NM / MD of the caller's requests on the caller's regions (include/ssgpu.h), through run_reg2aln as run_req_tail goes through it */
int ssg_dbg_reg2aln(const ssg_mem_opt_t *opt, const uint8_t *pac, int64_t l_pac, int n_ctg, const int64_t *ctg_off, const int32_t *ctg_len, int n_reads, const uint8_t *seq, const int64_t *off,
                    int64_t n_regs, const ssg_alnreg_t *regs, int64_t n_req, const ssg_alnreq_t *req, ssg_aln_t *alns, int32_t *route, int32_t *dev_err)
{
	CHK(ssg_need_device());
	if (dev_err) *dev_err = 0;
	if (n_reads < 0 || n_regs < 0 || n_req < 0 || n_req >= (int64_t)1 << 31 || l_pac < 1 || l_pac >= (int64_t)1 << 33 || n_ctg < 1) {
		ssg_err_msg = "ssg_dbg_reg2aln: need n_reads, n_regs >= 0, 0 <= n_req < 2^31, 1 <= l_pac < 2^33, n_ctg >= 1"; return SSG_EINVAL; }
	CHK(dbg_check_contigs("ssg_dbg_reg2aln", l_pac, n_ctg, ctg_off, ctg_len));
	if (n_req == 0) return SSG_OK;
	const char *bad = 0; long at = 0;
	int max_len = 0;
	if (n_reads < 1) bad = "requests need reads: request";
	else if (off[0] != 0) bad = "offsets start at 0: read";
	for (int r = 0; !bad && r < n_reads; ++r) {
		at = r;
		max_len = std::max(max_len, dbg_read_len(off, r, &bad));
		if (!bad) dbg_check_codes(seq, off, r, &bad);
	}
	for (int64_t k = 0; !bad && k < n_regs; ++k) {
		const ssg_alnreg_t &a = regs[k];
		at = (long)k;
		if (!(0 <= a.rb && a.rb < a.re && a.re <= 2 * l_pac)) bad = "need 0 <= rb < re <= 2 l_pac: region";
		else if (a.rb < l_pac && a.re > l_pac) bad = "a region must not cross the forward / reverse boundary l_pac: region";
		else if (a.re - a.rb > SSG_STAGE_TWIN_GLB) bad = "need re - rb <= 32768: region";
		else if (!(0 <= a.qb && a.qb < a.qe && a.qe <= SSG_MAX_READ_LEN)) bad = "need 0 <= qb < qe <= read length: region";
	}
	for (int64_t k = 0; !bad && k < n_req; ++k) {
		const ssg_alnreq_t &q = req[k];
		at = (long)k;
		if (q.read < 0 || q.read >= n_reads) bad = "read index out of range: request";
		else if (q.reg >= n_regs) bad = "region index out of range: request";
		else if (q.kind != SSG_REQ_MAIN && q.kind != SSG_REQ_XA) bad = "kind is SSG_REQ_MAIN or SSG_REQ_XA: request";
		else if (q.reg >= 0 && regs[q.reg].qe > off[q.read + 1] - off[q.read]) bad = "need 0 <= qb < qe <= read length for the request's region and read: request";
	}
	if (bad) return dbg_refuse("ssg_dbg_reg2aln", bad, at);
	/* the scoring limits of the pipeline (the functions run_align1, run_regions and run_reg2aln call), whatever the requests */
	CHK(check_band(opt)); CHK(check_scores(opt, max_len)); CHK(check_gap_penalties(opt));
	dbg_ref_t ref;
	CHK(ref.up(pac, l_pac, n_ctg, ctg_off, ctg_len));
	dbuf<uint8_t> d_seq((size_t)off[n_reads] + 1); dbuf<int64_t> d_off((size_t)n_reads + 1); dbuf<int32_t> d_gerr(1);
	dbuf<ssg_alnreg_t> d_regs((size_t)n_regs + 1); dbuf<ssg_alnreq_t> d_req((size_t)n_req + 1); dbuf<ssg_aln_t> d_alns((size_t)n_req + 1); dbuf<unsigned long long> d_cnt(3);
	CHKA(d_seq); CHKA(d_off); CHKA(d_gerr); CHKA(d_regs); CHKA(d_req); CHKA(d_alns); CHKA(d_cnt);
	CHK(d_seq.up(seq, (size_t)off[n_reads])); CHK(d_off.up(off, (size_t)n_reads + 1));
	if (n_regs) CHK(d_regs.up(regs, (size_t)n_regs));
	CHK(d_req.up(req, (size_t)n_req)); CHK(d_alns.zero()); CHK(d_gerr.zero()); CHK(d_cnt.zero());
	r2a_lists_t lists;
	CHK(run_reg2aln(ref.ix, opt, n_req, d_req.p, d_regs.p, d_seq.p, d_off.p, d_alns.p, d_gerr.p, d_cnt.p, max_len, &lists));
	int32_t ge = 0;
	CHK(d_gerr.down(&ge, 1));
	if (dev_err) *dev_err = ge;
	CHK(d_alns.down(alns, (size_t)n_req));
	if (route) {
		for (int64_t k = 0; k < n_req; ++k) route[k] = req[k].reg >= 0 ? SSG_R2A_ROUTE_LANE : 0;
		for (int c = 0; c < SSG_STAGE_R2D_CLASSES; ++c) for (int32_t g : lists.dp[c]) if (g >= 0 && g < n_req) route[g] = SSG_R2A_ROUTE_DP0 << c;
		for (int32_t g : lists.todo) if (g >= 0 && g < n_req) route[g] = (route[g] & ~SSG_R2A_ROUTE_LANE) | SSG_R2A_ROUTE_WAVE;
	}
	if (ge) { ssg_err_msg = "CIGAR generation exceeded an on-device capacity (code " + std::to_string(ge) + ")"; return SSG_EOVERFLOW; }
	return SSG_OK;
}

/* ---- test entries of the paired-end decision stage: region lists in, the stage's own results out (include/ssgpu.h) ---- */
static int dbg_check_regs(const ssg_index_t *idx, int n_pairs, const int64_t *reg_off, const ssg_alnreg_t *regs, const char *who)
{	/* the kernels index by what the lists say: nothing out of range may reach them */
	const int n_reads = 2 * n_pairs;
	const char *bad = 0; long at = -1;
	if (n_pairs < 0 || n_pairs > (1 << 24)) { bad = "n_pairs out of range"; at = n_pairs; }
	else if (reg_off[0] != 0) { bad = "reg_off[0] != 0"; at = 0; }
	for (int r = 0; r < n_reads && !bad; ++r) {
		if (reg_off[r + 1] < reg_off[r] || reg_off[r + 1] - reg_off[r] > 4096) { bad = "reg_off not monotone, or more than 4096 regions in a read: read"; at = r; }
		else if (reg_off[r + 1] > (1LL << 28)) { bad = "too many regions in all: read"; at = r; }
	}
	for (int64_t k = 0; !bad && k < reg_off[n_reads]; ++k) {
		const ssg_alnreg_t &e = regs[k];
		if (e.rid < 0 || e.rid >= idx->v.n_ctg) bad = "rid out of range: region";
		else if (!(0 <= e.qb && e.qb < e.qe && e.qe <= 310)) bad = "need 0 <= qb < qe <= 310: region";
		else if (!(0 <= e.rb && e.rb < e.re && e.re <= 2 * idx->v.l_pac)) bad = "need 0 <= rb < re <= 2 l_pac: region";
		else if (e.score < 0 || e.score > (1 << 20) || e.csub < 0 || e.csub > (1 << 20)) bad = "score / csub out of range: region";
		else if (!(e.frac_rep >= 0 && e.frac_rep <= 1)) bad = "frac_rep outside [0, 1]: region";
		if (bad) at = (long)k;
	}
	return bad ? dbg_refuse(who, bad, at) : 0;
}

int ssg_dbg_pestat(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_pairs, const int64_t *reg_off, const ssg_alnreg_t *regs,
                   const int32_t *pair_batch, int n_batches, ssg_pestat_t *pes)
{
	CHK(ssg_need_device());
	CHK(dbg_check_regs(idx, n_pairs, reg_off, regs, "ssg_dbg_pestat"));
	if (n_batches < 1 || n_batches > 64) { ssg_err_msg = "ssg_dbg_pestat: 1 <= n_batches <= 64"; return SSG_EINVAL; }
	for (int p = 0; p < n_pairs; ++p) if (pair_batch[p] < 0 || pair_batch[p] >= n_batches) { ssg_err_msg = "ssg_dbg_pestat: pair_batch out of range"; return SSG_EINVAL; }
	const int n_reads = 2 * n_pairs;
	const int64_t tot = reg_off[n_reads];
	const std::vector<int32_t> hn = dbg_counts(reg_off, n_reads);
	dbuf<int64_t> d_off((size_t)n_reads + 1); dbuf<ssg_alnreg_t> d_regs((size_t)tot + 1); dbuf<int32_t> d_n((size_t)n_reads + 1), d_pb((size_t)n_pairs + 1);
	CHKA(d_off); CHKA(d_regs); CHKA(d_n); CHKA(d_pb);
	CHK(d_off.up(reg_off, (size_t)n_reads + 1)); CHK(d_regs.up(regs, (size_t)tot)); CHK(d_n.up(hn.data(), (size_t)n_reads)); CHK(d_pb.up(pair_batch, (size_t)n_pairs));
	return run_pestat(idx, opt, n_pairs, d_off.p, d_regs.p, d_n.p, d_pb.p, n_batches, pes);
}

int ssg_dbg_pair_final(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_pairs, int64_t id0, const int64_t *reg_off, const ssg_alnreg_t *regs,
                       const ssg_pestat_t pes[4], ssg_alnreg_t *regs_out, int64_t *req_off, ssg_alnreq_t **req)
{
	CHK(ssg_need_device());
	CHK(dbg_check_regs(idx, n_pairs, reg_off, regs, "ssg_dbg_pair_final"));
	for (int d = 0; d < 4; ++d) if (!pes[d].failed && !(pes[d].std > 0 && pes[d].low >= 0 && pes[d].low <= pes[d].high)) { ssg_err_msg = "ssg_dbg_pair_final: an orientation that has not failed needs std > 0 and 0 <= low <= high"; return SSG_EINVAL; }
	const int n_reads = 2 * n_pairs;
	const int64_t tot = reg_off[n_reads];
	*req = 0;
	if (n_pairs == 0) { req_off[0] = 0; return SSG_OK; }
	const std::vector<int32_t> hn = dbg_counts(reg_off, n_reads);
	dbuf<int64_t> d_off((size_t)n_reads + 1); dbuf<ssg_alnreg_t> d_regs((size_t)tot + 1); dbuf<int32_t> d_n((size_t)n_reads), d_pb((size_t)n_pairs); dbuf<ssg_pestat_t> d_pes(4);
	CHKA(d_off); CHKA(d_regs); CHKA(d_n); CHKA(d_pb); CHKA(d_pes);
	CHK(d_off.up(reg_off, (size_t)n_reads + 1)); CHK(d_regs.up(regs, (size_t)tot)); CHK(d_n.up(hn.data(), (size_t)n_reads)); CHK(d_pb.zero()); CHK(d_pes.up(pes, 4));
	/* slices, request capacities and the heaviest-first order: the pipeline's own (make_pair_slices) */
	pair_slices_t s;
	CHK(make_pair_slices(n_reads, d_off.p, d_regs.p, d_n.p, opt->max_matesw, s));
	dbuf<int32_t> d_perr(n_pairs), d_zbuf((size_t)s.t2 + 1), d_nreq(n_reads); dbuf<unsigned int> d_q(1); dbuf<ssg_alnreq_t> d_req((size_t)s.tq + 1);
	CHKA(d_perr); CHKA(d_zbuf); CHKA(d_nreq); CHKA(d_q); CHKA(d_req);
	CHK(d_perr.zero()); CHK(d_nreq.zero());
	CHK(run_pair_final(idx, opt, n_pairs, id0, s.t2, s.d_r2off.p, s.d_regs2.p, d_n.p, d_pb.p, d_pes.p, s.d_pkey.p, s.d_pw.p, d_zbuf.p, s.d_reqoff.p, d_req.p, d_nreq.p, d_perr.p, d_q.p));
	/* the regions back into the caller's layout, the requests compacted by the pipeline's own tail (without its CIGAR step) */
	CHK(dev_copy_regs(n_reads, s.d_r2off.p, s.d_regs2.p, d_n.p, d_off.p, d_regs.p));
	pe_dev_t t;
	CHK(run_req_tail(n_reads, s.d_reqoff.p, d_req.p, d_nreq.p, 0, 0, t));
	CHK(rt_sync());
	const int64_t nreq = t.n_req;
	std::vector<int64_t> r2off((size_t)n_reads + 1);
	CHK(s.d_r2off.down(r2off.data(), (size_t)n_reads + 1)); CHK(t.req_off.down(req_off, (size_t)n_reads + 1)); CHK(d_regs.down(regs_out, (size_t)tot));
	ssg_alnreq_t *out = (ssg_alnreq_t*)malloc(sizeof(ssg_alnreq_t) * (size_t)(nreq + 1));
	if (!out) { ssg_err_msg = "host allocation failed: requests"; return SSG_ENOMEM; }
	int rc = t.req.down(out, (size_t)nreq);
	if (rc) { free(out); return rc; }
	for (int64_t k = 0; k < nreq; ++k) if (out[k].reg >= 0) out[k].reg = (int32_t)(out[k].reg - r2off[out[k].read] + reg_off[out[k].read]);   /* slice index -> the caller's index */
	*req = out;
	return SSG_OK;
}

int ssg_dbg_matesw(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_pairs, const uint8_t *seq, const int64_t *read_off, const int64_t *reg_off, const ssg_alnreg_t *regs,
                   const uint8_t *fixed, const ssg_pestat_t pes[4], int headroom, int64_t *out_off, ssg_alnreg_t **regs_out, int32_t *n_out, int32_t *err, uint64_t counts[8])
{
	CHK(ssg_need_device());
	CHK(dbg_check_regs(idx, n_pairs, reg_off, regs, "ssg_dbg_matesw"));
	for (int d = 0; d < 4; ++d) if (!pes[d].failed && !(pes[d].low >= 0 && pes[d].low <= pes[d].high)) { ssg_err_msg = "ssg_dbg_matesw: an orientation that has not failed needs 0 <= low <= high"; return SSG_EINVAL; }
	const int n_reads = 2 * n_pairs;
	*regs_out = 0; memset(counts, 0, 8 * sizeof(uint64_t));
	if (n_pairs == 0) { out_off[0] = 0; return SSG_OK; }
	int max_len = 0;
	for (int r = 0; r < n_reads; ++r) {
		if (read_off[r + 1] <= read_off[r] || (r == 0 && read_off[0] != 0)) { ssg_err_msg = "ssg_dbg_matesw: read_off must start at 0 and increase"; return SSG_EINVAL; }
		max_len = std::max<int>(max_len, (int)std::min<int64_t>(read_off[r + 1] - read_off[r], 1 << 20));
	}
	if (max_len > SSG_MAX_READ_LEN) { ssg_err_msg = "reads longer than " SSG_STR(SSG_MAX_READ_LEN) " bases are outside this build's scope"; return SSG_EINVAL; }
	for (int64_t k = 0; k < read_off[n_reads]; ++k) if (seq[k] > 4) { ssg_err_msg = "ssg_dbg_matesw: bases are codes 0 .. 4"; return SSG_EINVAL; }
	for (int r = 0; r < n_reads; ++r) for (int64_t k = reg_off[r]; k < reg_off[r + 1]; ++k) if (regs[k].qe > (int)(read_off[r + 1] - read_off[r])) { ssg_err_msg = "ssg_dbg_matesw: a region ends beyond its read"; return SSG_EINVAL; }
	/* the slices as ssg_k_pair_caps sizes them (own regions + 4 rescued hits per anchor of the mate + 4), or own regions + headroom */
	const std::vector<int32_t> hn = dbg_counts(reg_off, n_reads);
	std::vector<int32_t> hkey((size_t)n_pairs); std::vector<int64_t> r2off((size_t)n_reads + 1, 0); std::vector<uint8_t> hfix((size_t)n_reads, 0);
	for (int r = 0; r < n_reads; ++r) { const int m = hn[r ^ 1]; r2off[r + 1] = r2off[r] + hn[r] + (headroom >= 0 ? headroom : 4 * std::min(m, opt->max_matesw) + 4); if (fixed) hfix[r] = fixed[r] ? 1 : 0; }
	for (int p = 0; p < n_pairs; ++p) hkey[p] = hn[2 * p] + hn[2 * p + 1];
	const int64_t tot = reg_off[n_reads], t2 = r2off[n_reads];
	dbuf<uint8_t> d_seq((size_t)read_off[n_reads] + 1), d_fixed((size_t)n_reads); dbuf<int64_t> d_roff((size_t)n_reads + 1), d_off((size_t)n_reads + 1), d_r2off((size_t)n_reads + 1);
	dbuf<ssg_alnreg_t> d_regs((size_t)tot + 1), d_regs2((size_t)t2 + 1); dbuf<int32_t> d_n((size_t)n_reads), d_pb((size_t)n_pairs), d_pkey((size_t)n_pairs), d_pw((size_t)n_pairs), d_perr((size_t)n_pairs);
	dbuf<ssg_pestat_t> d_pes(4); dbuf<unsigned long long> d_cnt(3); dbuf<unsigned int> d_q(1);
	CHKA(d_seq); CHKA(d_fixed); CHKA(d_roff); CHKA(d_off); CHKA(d_r2off); CHKA(d_regs); CHKA(d_regs2); CHKA(d_n); CHKA(d_pb); CHKA(d_pkey); CHKA(d_pw); CHKA(d_perr); CHKA(d_pes); CHKA(d_cnt); CHKA(d_q);
	CHK(d_seq.up(seq, (size_t)read_off[n_reads])); CHK(d_fixed.up(hfix.data(), (size_t)n_reads)); CHK(d_roff.up(read_off, (size_t)n_reads + 1)); CHK(d_off.up(reg_off, (size_t)n_reads + 1));
	CHK(d_r2off.up(r2off.data(), (size_t)n_reads + 1)); CHK(d_regs.up(regs, (size_t)tot)); CHK(d_regs2.zero()); CHK(d_n.up(hn.data(), (size_t)n_reads)); CHK(d_pb.zero()); CHK(d_pkey.up(hkey.data(), (size_t)n_pairs));
	CHK(d_perr.zero()); CHK(d_pes.up(pes, 4)); CHK(d_cnt.zero()); CHK(d_q.zero());
	CHK(dev_order_desc(d_pkey.p, d_pw.p, n_pairs)); CHK(rt_sync());
	CHK(dev_copy_regs(n_reads, d_off.p, d_regs.p, d_n.p, d_r2off.p, d_regs2.p));
	msw_stage_t ms;
	CHK(run_matesw(idx, opt, n_pairs, d_seq.p, d_roff.p, max_len, d_r2off.p, d_regs2.p, d_n.p, d_pb.p, d_pes.p, d_pw.p, d_fixed.p, d_perr.p, d_cnt.p, d_q.p, &ms));
	ssg_alnreg_t *out = (ssg_alnreg_t*)malloc(sizeof(ssg_alnreg_t) * (size_t)(t2 + 1));
	if (!out) { ssg_err_msg = "host allocation failed: regions"; return SSG_ENOMEM; }
	int rc = d_regs2.down(out, (size_t)t2);
	if (!rc) rc = d_n.down(n_out, (size_t)n_reads);
	if (!rc) rc = d_perr.down(err, (size_t)n_pairs);
	if (rc) { free(out); return rc; }
	memcpy(out_off, r2off.data(), ((size_t)n_reads + 1) * sizeof(int64_t));
	msw_counts(ms, counts);
	*regs_out = out;
	return SSG_OK;
}

/* test entry: one bwt_extend per item by the seeding kernels' two forms (include/ssgpu.h); the kernel is ssg_seed.cpp's */
int ssg_dbg_extend_coop(const ssg_index_t *idx, int n, const ssg_intv_t *in, const uint8_t *base, const uint8_t *is_back, ssg_intv_t *out_lean, ssg_intv_t *out_coop,
                        ssg_intv_t *out_lean4, ssg_intv_t *out_coop4)
{
	CHK(ssg_need_device());
	if (n < 0 || n > 1 << 24) { ssg_err_msg = "ssg_dbg_extend_coop: need 0 <= n <= 2^24"; return SSG_EINVAL; }
	if (n == 0) return SSG_OK;
	const uint64_t seq_len = idx->v.seq_len;
	std::vector<uint8_t> cd((size_t)n);
	for (int t = 0; t < n; ++t) {
		if (base[t] > 3) return dbg_refuse("ssg_dbg_extend_coop", "bases are codes 0 .. 3: item", t);
		if (is_back[t] > 1) return dbg_refuse("ssg_dbg_extend_coop", "is_back is 0 or 1: item", t);
		/* the rank queries are rows kx - 1 (-1 allowed) and kx - 1 + x2 of the text with its sentinel: rows 0 .. seq_len; an item's interval is also extended
		 * in its neighbours' direction (the four-interval form), so both sides must do */
		for (int side = 0; side < 2; ++side) {
			const uint64_t kx = side ? in[t].x0 : in[t].x1;
			if (kx > seq_len + 1 || in[t].x2 > seq_len + 1 || kx + in[t].x2 > seq_len + 1) return dbg_refuse("ssg_dbg_extend_coop", "need x0 + x2 <= text length + 1 and x1 + x2 <= text length + 1: item", t);
		}
		cd[t] = (uint8_t)(base[t] | is_back[t] << 2);
	}
	dbuf<ssg_intv_t> d_in((size_t)n), d_lean((size_t)n), d_coop((size_t)n), d_lean4((size_t)n * 4), d_coop4((size_t)n * 4); dbuf<uint8_t> d_cd((size_t)n);
	CHKA(d_in); CHKA(d_lean); CHKA(d_coop); CHKA(d_lean4); CHKA(d_coop4); CHKA(d_cd);
	CHK(d_in.up(in, (size_t)n)); CHK(d_cd.up(cd.data(), (size_t)n)); CHK(d_lean.zero()); CHK(d_coop.zero()); CHK(d_lean4.zero()); CHK(d_coop4.zero());
	CHK(ssg_seed_dbg_extend_coop(idx, n, d_in.p, d_cd.p, d_lean.p, d_coop.p, d_lean4.p, d_coop4.p));
	CHK(d_lean.down(out_lean, (size_t)n)); CHK(d_coop.down(out_coop, (size_t)n)); CHK(d_lean4.down(out_lean4, (size_t)n * 4));
	return d_coop4.down(out_coop4, (size_t)n * 4);
}

/* test entry: the seeding kernels on the caller's reads with the extension count (include/ssgpu.h), through ssg_seed_smem2 as the pipeline's seeding stage goes through it */
int ssg_dbg_smem_ext(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_reads, const uint8_t *seq, const int64_t *off, int cap, ssg_intv_t *out_intv, int32_t *out_n, uint64_t *n_extend, uint32_t paths[4])
{
	CHK(ssg_need_device());
	*n_extend = 0; memset(paths, 0, 4 * sizeof(uint32_t));
	if (n_reads < 0 || cap < 1) { ssg_err_msg = "ssg_dbg_smem_ext: need n_reads >= 0, cap >= 1"; return SSG_EINVAL; }
	if (n_reads == 0) return SSG_OK;
	if (off[0] != 0) return dbg_refuse("ssg_dbg_smem_ext", "offsets start at 0: read", 0);
	int max_len = 0;
	for (int r = 0; r < n_reads; ++r) {
		const char *bad = 0;
		const int64_t len = off[r + 1] - off[r];   /* (an empty read is a read: ssg_smem_batch takes it) */
		if (len < 0) bad = "offsets must not decrease: read";
		else if (len > SSG_MAX_READ_LEN) bad = "need read length <= " SSG_STR(SSG_MAX_READ_LEN) ": read";
		if (!bad) dbg_check_codes(seq, off, r, &bad);
		if (bad) return dbg_refuse("ssg_dbg_smem_ext", bad, r);
		max_len = std::max(max_len, (int)len);
	}
	const char *e = getenv("SSG_SMEM_MAX_EXT");
	const unsigned int max_ext = e && *e ? (unsigned int)atoi(e) : (unsigned int)(13 * max_len + 50);   /* the seeding stage's own default */
	dbuf<uint8_t> d_seq((size_t)off[n_reads] + 1); dbuf<int64_t> d_off((size_t)n_reads + 1); dbuf<ssg_intv_t> d_intv((size_t)n_reads * cap); dbuf<int32_t> d_n((size_t)n_reads); dbuf<unsigned long long> d_nx(1); dbuf<unsigned int> d_paths(4);
	CHKA(d_seq); CHKA(d_off); CHKA(d_intv); CHKA(d_n); CHKA(d_nx); CHKA(d_paths);
	CHK(d_seq.up(seq, (size_t)off[n_reads])); CHK(d_off.up(off, (size_t)n_reads + 1)); CHK(d_nx.zero()); CHK(d_paths.zero());
	CHK(ssg_seed_smem2_paths(idx, opt, n_reads, d_seq.p, d_off.p, max_len, cap, d_intv.p, d_n.p, d_nx.p, max_ext, d_paths.p));
	unsigned long long nx = 0;
	CHK(d_nx.down(&nx, 1)); CHK(d_intv.down(out_intv, (size_t)n_reads * cap)); CHK(d_n.down(out_n, (size_t)n_reads));
	for (int r = 0; r < n_reads; ++r) if (out_n[r] < 0) { ssg_err_msg = "ssg_dbg_smem_ext: a read's list exceeds the per-read capacity"; return SSG_EOVERFLOW; }
	*n_extend = nx;
	return d_paths.down(paths, 4);
}

/* test entry: samblaster's stage of the timed step on the caller's records (include/ssgpu.h), through the host functions ssg_hotpath_dev_ex runs after alignment */
int ssg_dbg_sbl_records(long n_pairs, const int64_t *req_off, const ssg_alnreq_t *req, const ssg_aln_t *alns, const ssg_sbl_opt_t *o, ssg_sbl_state_t *st,
                        int64_t *line_off, int64_t *n_lines, ssg_sbl_line_t *lines, int64_t *line_req, ssg_sbl_end_t *ends, int64_t *prim, uint64_t *sig, uint8_t *dup,
                        uint8_t *bits, int64_t *mate_line, uint64_t counts[4], uint64_t *keys)
{
	const char *who = "ssg_dbg_sbl_records";
	CHK(ssg_need_device());
	*n_lines = 0; memset(counts, 0, 4 * sizeof(uint64_t));
	if (n_pairs < 0 || n_pairs >= (1L << 31)) { ssg_err_msg = "ssg_dbg_sbl_records: need 0 <= n_pairs < 2^31"; return SSG_EINVAL; }
	if (o->max_split_count > SSG_STAGE_SBL_MAX_SPLIT) { ssg_err_msg = "samblaster: --maxSplitCount above 16 is not supported"; return SSG_EINVAL; }
	if (n_pairs == 0) { line_off[0] = 0; return SSG_OK; }
	if (req_off[0] != 0) return dbg_refuse(who, "offsets start at 0: read", 0);
	const long n_reads = 2 * n_pairs;
	for (long r = 0; r < n_reads; ++r) {
		if (req_off[r + 1] < req_off[r]) return dbg_refuse(who, "offsets must not decrease: read", r);
		int n_main = 0;
		for (int64_t g = req_off[r]; g < req_off[r + 1]; ++g) {
			if (req[g].kind != SSG_REQ_MAIN && req[g].kind != SSG_REQ_XA) return dbg_refuse(who, "kind is SSG_REQ_MAIN or SSG_REQ_XA: request", (long)g);
			if (alns[g].n_cigar < 0 || alns[g].n_cigar > SSG_MAX_CIGAR) return dbg_refuse(who, "need 0 <= n_cigar <= " SSG_STR(SSG_MAX_CIGAR) ": record", (long)g);
			n_main += req[g].kind == SSG_REQ_MAIN;
		}
		if (!n_main) return dbg_refuse(who, "a read without a main request: read", r);
		if (req[req_off[r]].kind != SSG_REQ_MAIN) return dbg_refuse(who, "the first request of a read is a main one (its mate's lines print against it): read", r);
	}
	const size_t nreq = (size_t)req_off[n_reads];
	dbuf<int64_t> d_off((size_t)n_reads + 1); dbuf<ssg_alnreq_t> d_req(nreq + 1); dbuf<ssg_aln_t> d_alns(nreq + 1); dbuf<uint64_t> d_sig(3 * (size_t)n_pairs);
	CHKA(d_off); CHKA(d_req); CHKA(d_alns); CHKA(d_sig);
	CHK(d_off.up(req_off, (size_t)n_reads + 1)); CHK(d_req.up(req, nreq)); CHK(d_alns.up(alns, nreq));
	sbl_lines_t L;
	CHK(records_lines(n_pairs, d_off.p, d_req.p, d_alns.p, &L));
	CHK(records_dedup(st, n_pairs, L.ends.p, L.dup.p, d_sig.p));
	CHK(records_classify(n_pairs, &L, o, L.dup.p, counts));
	const size_t nl = (size_t)L.n_lines;
	dbuf<uint64_t> d_keys(nl + 1);
	CHKA(d_keys);
	CHK(records_export(&L, d_alns.p, d_keys.p, 0, 0));
	*n_lines = L.n_lines;
	CHK(L.line_off.down(line_off, (size_t)n_pairs + 1)); CHK(L.lines.down(lines, nl)); CHK(L.line_req.down(line_req, nl)); CHK(L.ends.down(ends, 2 * (size_t)n_pairs));
	CHK(L.prim.down(prim, 2 * (size_t)n_pairs)); CHK(d_sig.down(sig, 3 * (size_t)n_pairs)); CHK(L.dup.down(dup, (size_t)n_pairs)); CHK(L.bits.down(bits, nl));
	CHK(L.mate.down(mate_line, nl));
	return d_keys.down(keys, nl);
}
