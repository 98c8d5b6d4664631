/*
 * ssg_msw_replay.cpp -- the launcher of ssg_k_matesw_keys (k_mswkeys.h): mate rescue's list logic replayed on compact keys, for the pairs all of whose
 * windows were aligned ahead of the decision.  A translation unit of its own: a kernel added to ssgpu_core.cpp would be compiled next to kernels whose
 * machine code is pinned (tools/isa_pin.py), and this one includes no header that holds a kernel of another unit.
 */
#include <algorithm>
#include "ssg_rt.h"
#include "k_mswkeys.h"
#include "../../include/ssgpu.h"
#include "ssg_index_int.h"
#include "ssg_pe_int.h"

SSG_ABI_FP_DEFINE(msw_replay)
static_assert(SSG_MSW_NCNT == SSG_MK_NCNT, "ssg_pe_int.h and k_mswkeys.h disagree about the counters");

size_t ssg_msw_replay_scratch(long n_waves, size_t *slab_bytes)
{
	*slab_bytes = (size_t)n_waves * sizeof(ssg_mk_big_t);
	return (size_t)n_waves * SSG_MK_BIGCAP;
}

long ssg_msw_replay_waves(unsigned int n_todo, int max_wgs)
{
	const long nwg = std::min<long>(((long)n_todo + SSG_MK_WAVES - 1) / SSG_MK_WAVES, std::max(max_wgs, 1));
	return nwg * SSG_MK_WAVES;
}

int ssg_msw_replay(const ssg_index *idx, const ssg_mem_opt_t *opt, long n_waves, const int32_t *d_todo, const unsigned int *d_ntodo, const int64_t *d_off,
                   const int64_t *d_r2off, ssg_alnreg_t *d_regs2, int32_t *d_nreg, const int32_t *d_pb, const ssg_pestat_t *d_pes,
                   ssg_alnreg_t *d_tmp, void *d_slab, unsigned int *d_q, unsigned long long *d_cells, unsigned long long *d_nrescue,
                   const ssg_msres_t *d_jres, const int64_t *d_jbase, const uint8_t *d_fixed, int tcap, int32_t *d_left, int64_t *d_lbase, unsigned int *d_cnt)
{
	if (n_waves <= 0) return 0;
	CHK(rt_memset(d_q, 0, sizeof(unsigned int))); CHK(rt_memset(d_cnt, 0, SSG_MK_NCNT * sizeof(unsigned int)));
	SSG_LAUNCH(ssg_k_matesw_keys, n_waves / SSG_MK_WAVES, SSG_MK_WAVES * 64, 0, idx->v, *opt, d_off, d_r2off, d_regs2, d_nreg, d_pb, d_pes, d_tmp, (ssg_mk_big_t*)d_slab,
	           d_cells, d_nrescue, d_todo, d_ntodo, d_q, d_jres, d_jbase, d_fixed, tcap, d_left, d_lbase, d_cnt);
	return 0;
}
