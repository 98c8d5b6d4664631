/*
 * k_mswslot.h -- what the kernels of the mate-rescue stage share without sharing device code: the orientation test of upstream mem_infer_dir and the
 * job / result records of the windows computed ahead of the decision (k_mswlane.h writes the slots; k_pair.h and k_mswkeys.h read them).  No kernels here:
 * a translation unit that includes this header gets none of its neighbours' machine code.
 */
#ifndef SSG_K_MSWSLOT_H
#define SSG_K_MSWSLOT_H
#include "ssg_dev.h"

SSG_DEVFN int ssg_infer_dir(int64_t l_pac, int64_t b1, int64_t b2, int64_t *dist)
{	/* upstream mem_infer_dir */
	int r1 = (b1 >= l_pac), r2 = (b2 >= l_pac);
	int64_t p2 = r1 == r2 ? b2 : (l_pac << 1) - 1 - b2;
	*dist = p2 > b1 ? p2 - b1 : b1 - p2;
	return (r1 == r2 ? 0 : 1) ^ (p2 > b1 ? 0 : 3);
}

/* slot = side base + 4 * anchor + orientation.  p = 16 / 8: the padding unit of the query (KSW_XBYTE or not); xstart: KSW_XSTART */
struct ssg_msjob_t { int64_t rb, qoff; int32_t tlen, qlen, qp, minsc, is_rev, p, xstart, _pad; };                 /* 48 bytes */
struct ssg_msres_t { int64_t rb; int32_t tlen, state, score, te, qe, score2, te2, tb, qb, _pad; };   /* 48 bytes; state: 0 = not computed, 1 = forward pass, 2 = forward and reverse pass (tb, qb) */
#endif
