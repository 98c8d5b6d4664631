/*
 * ssg_recs_int.h -- the record store shared by the translation units that work on it (ssg_rec_gather.cpp: create / append / order / gather / reopen /
 * release / free; ssg_bam_scan.cpp: BGZF members inflated into a chunk, the records of a chunk found on the device).
 */
#ifndef SSG_RECS_INT_H
#define SSG_RECS_INT_H
#include <string>
#include <vector>
#include "ssg_rt.h"
#include "../../include/ssgpu.h"

/* the device mirror of the sort's record store (rec_store_t, sambamba_main.cpp): a chunk is a device allocation of its own, outside the arena -- gigabytes
 * that go back to the driver with the store -- with 16 bytes of slack behind it, so that a 16-byte load that starts inside a record stays inside.  A released
 * chunk (ssg_recs_release) keeps its id: d_chunk[id] = NULL, len[id] = 0 */
struct ssg_recs {
	int dev; uint64_t cap, bytes;
	std::vector<uint8_t*> d_chunk; std::vector<uint64_t> len;
	/* what ssg_recs_order leaves for the kernel */
	bool ordered; int64_t n; uint64_t total;
	uint8_t **d_ptr; uint64_t *d_loc, *d_cum;
	ssg_recs() : dev(0), cap(0), bytes(0), ordered(false), n(0), total(0), d_ptr(0), d_loc(0), d_cum(0) {}
};
static inline void recs_drop_order(ssg_recs *r)
{
	rt_free_raw(r->d_ptr); rt_free_raw(r->d_loc); rt_free_raw(r->d_cum);
	r->d_ptr = 0; r->d_loc = r->d_cum = 0; r->ordered = false; r->n = 0; r->total = 0;
}
static inline int recs_usable(const ssg_recs *r, const char *who)
{
	if (rt_device_count() < 1) { ssg_err_msg = "no HIP device visible: libssgpu has no CPU path"; return SSG_ENODEV; }
	if (!r) { ssg_err_msg = std::string(who) + ": no record store"; return SSG_EINVAL; }
	if (r->dev != ssg_cur_dev) { ssg_err_msg = std::string(who) + ": the record store lives on device " + std::to_string(r->dev) + ", the calling thread drives device " + std::to_string(ssg_cur_dev); return SSG_EINVAL; }
	return 0;
}
/* what the kernels that run a filter program rely on (sel_keep, k_bam_select.h): every operation is known, finds its operands on the stack, and the program never
 * holds more than 64 values and leaves exactly one.  `who': the entry's name with ": " behind it */
static inline int recs_prog_ok(const std::string &who, const ssg_bam_fop_t *prog, int n_prog)
{
	if (n_prog < 0 || (n_prog > 0 && !prog)) { ssg_err_msg = who + "n_prog < 0, or no prog[]"; return SSG_EINVAL; }
	if (n_prog > SSG_FOP_MAX) { ssg_err_msg = who + "a filter program of " + std::to_string(n_prog) + " operations, at most " + std::to_string(SSG_FOP_MAX) + " are taken"; return SSG_EINVAL; }
	int depth = 0;
	for (int pc = 0; pc < n_prog; ++pc) {
		const ssg_bam_fop_t &f = prog[pc];
		if (f.op == SSG_FOP_AND || f.op == SSG_FOP_OR) { if (depth < 2) { ssg_err_msg = who + "operation " + std::to_string(pc) + " underflows the stack"; return SSG_EINVAL; } --depth; }
		else if (f.op == SSG_FOP_NOT) { if (depth < 1) { ssg_err_msg = who + "operation " + std::to_string(pc) + " underflows the stack"; return SSG_EINVAL; } }
		else if (f.op == SSG_FOP_FLAG) ++depth;
		else if (f.op >= SSG_FOP_EQ && f.op <= SSG_FOP_GE) {
			if (f.arg > SSG_FLD_FLAG) { ssg_err_msg = who + "operation " + std::to_string(pc) + " compares the unknown field " + std::to_string(f.arg); return SSG_EINVAL; }
			++depth;
		} else { ssg_err_msg = who + "operation " + std::to_string(pc) + " is the unknown operation " + std::to_string(f.op); return SSG_EINVAL; }
	}
	if (n_prog > 0 && depth != 1) { ssg_err_msg = who + "the filter program leaves " + std::to_string(depth) + " values, not exactly one"; return SSG_EINVAL; }
	return 0;
}
/* ssg_recs_scan with loc, key and ent of the chunk's records left in device memory (ssg_bam_scan.cpp): every check, state and message of the scan, the messages
 * under the caller's name `who'.  `arrays': the caller has a place for records (without one, a chunk that holds records is SSG_EINVAL, as the scan says it).
 * o.loc / o.key / o.ent hold *n_rec elements when 0 is returned and *n_rec > 0. */
struct recs_scan_dev_t { dbuf<uint64_t> loc, key; dbuf<ssg_bam_ent_t> ent; };
int recs_scan_dev(ssg_recs *r, const char *who, uint32_t chunk_id, const uint64_t *hint, int64_t n_hints, uint64_t first, uint64_t cap, bool arrays, uint64_t *n_rec, recs_scan_dev_t &o);
#endif
