/*
 * ssg_bam_select.cpp -- ssg_recs_select: ssg_recs_scan with the decision behind it (k_bam_select.h; the reader in the
 * reference: a region iterator's overlap test, htslib hts_itr_next, and the flag / MAPQ tests of `samtools view').  The scan is the scan's own host code
 * (recs_scan_dev, ssg_bam_scan.cpp) with loc, key and ent left in device memory; the regions and the filter program are checked here, so the kernel has
 * nothing to refuse.  A translation unit of its own: the machine code of the pinned kernels does not move (tools/isa_pin.py).
 */
#include <string>
#include <vector>
#include "ssg_rt.h"
#include "k_bam_select.h"
#include "ssg_prim.h"
#include "../../include/ssgpu.h"
#include "ssg_recs_int.h"

/* what the kernel relies on: regions sorted by (tid, beg), not empty, disjoint and not adjacent; a program whose every operation is known, finds its operands on
 * the stack, never holds more than 64 values and leaves exactly one */
static int select_args_ok(const ssg_bam_region_t *reg, int64_t n_reg, const ssg_bam_fop_t *prog, int n_prog)
{
	const std::string who = "ssg_recs_select: ";
	if (n_reg < 0 || n_reg > 0x7fffffff || (n_reg > 0 && !reg)) { ssg_err_msg = who + "n_reg < 0 or above 2^31 - 1, or no reg[]"; return SSG_EINVAL; }
	for (int64_t k = 0; k < n_reg; ++k) {
		const ssg_bam_region_t &g = reg[k];
		if (g.tid < 0 || g.beg < 0 || g.beg >= g.end) { ssg_err_msg = who + "region " + std::to_string(k) + " has tid < 0, beg < 0 or beg >= end"; return SSG_EINVAL; }
		if (k > 0 && (reg[k - 1].tid > g.tid || (reg[k - 1].tid == g.tid && reg[k - 1].end >= g.beg))) {
			ssg_err_msg = who + "region " + std::to_string(k) + " is not behind region " + std::to_string(k - 1) + ": the regions must be sorted by (tid, beg), disjoint and not adjacent";
			return SSG_EINVAL;
		}
	}
	return recs_prog_ok(who, prog, n_prog);
}

extern "C" {

int ssg_recs_select(ssg_recs_t *r, uint32_t chunk_id, const uint64_t *hint, int64_t n_hints, uint64_t first, const ssg_bam_region_t *reg, int64_t n_reg, const ssg_bam_fop_t *prog, int n_prog,
                    uint64_t cap, uint64_t *n_rec, uint64_t *n_sel, uint64_t *loc, uint64_t *key, ssg_bam_ent_t *ent)
{
	CHK(recs_usable(r, "ssg_recs_select"));
	if (!n_rec || !n_sel) { ssg_err_msg = "ssg_recs_select: no place for the number of records"; return SSG_EINVAL; }
	*n_rec = *n_sel = 0;
	if (r->ordered) { ssg_err_msg = "ssg_recs_select: refused while an order is declared: ssg_recs_reopen first"; return SSG_EINVAL; }
	const bool arrays = loc && key && ent, counting = cap == 0 && !loc && !key && !ent;
	if (!arrays && !counting) { ssg_err_msg = "ssg_recs_select: no loc[] / key[] / ent[] (all three NULL and cap == 0 is the counting form)"; return SSG_EINVAL; }
	CHK(select_args_ok(reg, n_reg, prog, n_prog));
	recs_scan_dev_t s;
	CHK(recs_scan_dev(r, "ssg_recs_select", chunk_id, hint, n_hints, first, ~(uint64_t)0, true, n_rec, s));
	const uint64_t n = *n_rec;
	if (n == 0) return 0;
	const uint64_t grid = (n + 255) / 256;   /* (below 2^31: the scan has checked it) */
	int32_t n_steps = 0;
	while (((int64_t)1 << n_steps) <= n_reg) ++n_steps;
	dbuf<ssg_bam_region_t> d_reg((size_t)n_reg + 1); dbuf<ssg_bam_fop_t> d_prog((size_t)n_prog + 1);
	dbuf<uint32_t> d_cnt((size_t)grid + 1); dbuf<uint64_t> d_base((size_t)grid + 1);
	if (!d_reg.ok() || !d_prog.ok() || !d_cnt.ok() || !d_base.ok()) { ssg_err_msg = "device allocation failed: the regions and counts of a selection"; return SSG_ENOMEM; }
	if (n_reg) CHK(d_reg.up(reg, (size_t)n_reg));
	if (n_prog) CHK(d_prog.up(prog, (size_t)n_prog));
	CHK(rt_memset(d_cnt.p + grid, 0, 4));   /* (one count more: the scan's last value is the total) */
	const uint8_t *const d_chunk = r->d_chunk[chunk_id];
	SSG_LAUNCH(ssg_k_bam_select, grid, 256, 0, d_chunk, (const uint64_t*)s.loc.p, (const uint64_t*)s.key.p, (const ssg_bam_ent_t*)s.ent.p, (int64_t)n, (const ssg_bam_region_t*)d_reg.p, (int32_t)n_reg, n_steps,
	           (const ssg_bam_fop_t*)d_prog.p, (int32_t)n_prog, d_cnt.p, (const uint64_t*)0, (uint64_t)0, (uint64_t*)0, (uint64_t*)0, (ssg_bam_ent_t*)0);
	CHK((prim_exsum<uint32_t, uint64_t>(d_cnt.p, d_base.p, (int64_t)grid + 1)));
	CHK(rt_sync());
	uint64_t m = 0; CHK(rt_d2h(&m, d_base.p + grid, 8));
	*n_sel = m;
	if (counting || m == 0) return 0;
	if (m > cap) { ssg_err_msg = "ssg_recs_select: " + std::to_string(m) + " records kept, room for " + std::to_string(cap); return SSG_EOVERFLOW; }
	dbuf<uint64_t> d_loc((size_t)m), d_key((size_t)m); dbuf<ssg_bam_ent_t> d_ent((size_t)m);
	if (!d_loc.ok() || !d_key.ok() || !d_ent.ok()) { ssg_err_msg = "device allocation failed: the records of a selection"; return SSG_ENOMEM; }
	SSG_LAUNCH(ssg_k_bam_select, grid, 256, 0, d_chunk, (const uint64_t*)s.loc.p, (const uint64_t*)s.key.p, (const ssg_bam_ent_t*)s.ent.p, (int64_t)n, (const ssg_bam_region_t*)d_reg.p, (int32_t)n_reg, n_steps,
	           (const ssg_bam_fop_t*)d_prog.p, (int32_t)n_prog, d_cnt.p, (const uint64_t*)d_base.p, m, d_loc.p, d_key.p, d_ent.p);
	CHK(rt_sync());
	CHK(d_loc.down(loc, (size_t)m)); CHK(d_key.down(key, (size_t)m)); CHK(d_ent.down(ent, (size_t)m));
	return 0;
}

} /* extern "C" */
