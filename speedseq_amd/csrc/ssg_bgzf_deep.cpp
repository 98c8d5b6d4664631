/*
 * ssg_bgzf_deep.cpp -- BGZF deflate on the device at levels 7-9 (k_bgzf_deep.h): the launcher ssg_bgzf.cpp puts in the place of ssg_k_bgzf_deflate when a
 * caller asks for one of those levels.  A translation unit of its own: a kernel added to ssg_bgzf.cpp would be compiled next to ssg_k_bgzf_deflate, whose
 * machine code is pinned (tools/isa_pin.py).
 */
#include "ssg_rt.h"
#include "k_bgzf_deep.h"
#include "../../include/ssgpu.h"
#include "ssg_index_int.h"

extern "C" {

/* candidates per position at a level: 0 = the level is not this unit's (1..6: ssg_k_bgzf_deflate) */
int ssg_bgzf_deep_depth(int level) { return level == 7 ? BZD_DEPTH_7 : level == 8 ? BZD_DEPTH_8 : level == 9 ? BZD_DEPTH_9 : 0; }
/* bytes of link scratch ssg_bgzf_deflate_deep_dev needs for nb blocks */
size_t ssg_bgzf_deep_scratch(long nb) { return (size_t)(nb > 0 ? nb : 0) * BZD_PREV_STRIDE * sizeof(uint16_t); }

/* queued on the calling thread's stream, behind what it has queued before; device buffers, those of ssg_k_bgzf_deflate plus d_prev (ssg_bgzf_deep_scratch) */
int ssg_bgzf_deflate_deep_dev(const uint8_t *d_pay, const uint64_t *d_cut, long nb, uint8_t *d_tmp, uint32_t *d_sym, uint32_t *d_size, uint16_t *d_prev, int depth)
{
	if (depth < 1 || !d_prev) { ssg_err_msg = "ssg_bgzf_deflate_deep_dev: no search depth or no link scratch"; return SSG_EINVAL; }
	SSG_LAUNCH(ssg_k_bgzf_deflate_deep, nb, 64, 0, d_pay, d_cut, (int)nb, d_tmp, d_sym, d_size, d_prev, depth);
	return 0;
}

} /* extern "C" */
