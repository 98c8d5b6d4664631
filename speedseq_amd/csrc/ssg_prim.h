/*
 * ssg_prim.h -- device-wide primitives used by the host orchestration: rocPRIM (AMD's own device library; no CUB-compatibility
 * layer) on the MI355X; plain loops in the host-emulation build (tests/emu, CPU-side tests only).  64-bit item counts.
 *
 * Every primitive is queued on the calling thread's stream (ssg_stream) and returns without waiting for it: the temporary goes back
 * to the lane's arena on return, and the arena hands it to the next request in stream order (ssg_rt.h, "Lanes").  A caller that reads
 * the result on the host, or frees memory that does not go through the arena, waits first (rt_sync, or a download).  The two
 * primitives that hand a count to the host -- prim_count_flags, prim_select -- end in that download.
 */
#ifndef SSG_PRIM_H
#define SSG_PRIM_H
#include "ssg_rt.h"
#include "ssg_dev.h"
#include "../../include/ssgpu.h"
#ifndef SSG_EMU
#include <rocprim/rocprim.hpp>
#else
#include <algorithm>
#include <vector>
#endif

#ifndef SSG_EMU
/* what all of them share: run(NULL, bytes, stream) asks for the size of the temporary, run(tmp, bytes, stream) queues the work */
template <class F> static inline int prim_run(const char *what, F run)
{
	size_t tb = 0;
	hipError_t e = run((void*)0, tb, ssg_stream);
	if (e == hipSuccess) {
		dbuf<uint8_t> tmp(tb);
		if (!tmp.ok()) { ssg_err_msg = std::string("device allocation failed: temporaries of ") + what; return SSG_ENOMEM; }
		e = run((void*)tmp.p, tb, ssg_stream);
	}
	if (e == hipSuccess) return 0;
	ssg_err_msg = std::string(what) + " failed: " + hipGetErrorString(e);
	(void)hipGetLastError();
	return SSG_EHIP;
}
template <class T> struct prim_max { SSG_DEVMEM T operator()(const T &a, const T &b) const { return a > b ? a : b; } };
template <class TI, class TO> struct prim_widen { SSG_DEVMEM TO operator()(const TI &v) const { return (TO)v; } };
#else
/* the bits [b0, b1) of a key, in place */
template <class K> static inline K prim_key_bits(K k, int b0, int b1) { return k & (K)((b1 >= (int)(8 * sizeof(K)) ? ~(K)0 : ((K)1 << b1) - 1) & ~(((K)1 << b0) - 1)); }
#endif

/* The sorts take their inputs as KI / VI = K* / V* or const K* / const V*, whichever the caller holds: rocPRIM instantiates its kernels per iterator type, and a
 * first pass that reads through the same pointer type as the later passes (which go from one buffer of K* to the other) shares their kernels. */
/* stable radix sort of keys on key bits [b0, b1) */
template <class KI, class K> static inline int prim_sort_keys(KI k_in, K *k_out, int64_t n, int b0, int b1)
{
	if (n <= 0) return 0;
#ifdef SSG_EMU
	std::vector<K> v(k_in, k_in + n);
	std::stable_sort(v.begin(), v.end(), [&](K a, K b) { return prim_key_bits(a, b0, b1) < prim_key_bits(b, b0, b1); });
	std::copy(v.begin(), v.end(), k_out);
	return 0;
#else
	return prim_run("rocprim radix_sort_keys", [&](void *tmp, size_t &tb, hipStream_t s) { return rocprim::radix_sort_keys(tmp, tb, k_in, k_out, (size_t)n, (unsigned)b0, (unsigned)b1, s); });
#endif
}

/* stable radix sort of (key, value), ascending, on key bits [b0, b1) */
template <class KI, class K, class VI, class V> static inline int prim_sort_pairs(KI k_in, K *k_out, VI v_in, V *v_out, int64_t n, int b0, int b1)
{
	if (n <= 0) return 0;
#ifdef SSG_EMU
	std::vector<int64_t> ix((size_t)n);
	for (int64_t i = 0; i < n; ++i) ix[(size_t)i] = i;
	std::stable_sort(ix.begin(), ix.end(), [&](int64_t a, int64_t b) { return prim_key_bits(k_in[a], b0, b1) < prim_key_bits(k_in[b], b0, b1); });
	for (int64_t i = 0; i < n; ++i) { k_out[i] = k_in[ix[(size_t)i]]; v_out[i] = v_in[ix[(size_t)i]]; }
	return 0;
#else
	return prim_run("rocprim radix_sort_pairs", [&](void *tmp, size_t &tb, hipStream_t s) { return rocprim::radix_sort_pairs(tmp, tb, k_in, k_out, v_in, v_out, (size_t)n, (unsigned)b0, (unsigned)b1, s); });
#endif
}

/* stable radix sort of (key, value) by the whole key, descending */
template <class KI, class K, class VI, class V> static inline int prim_sort_pairs_desc(KI k_in, K *k_out, VI v_in, V *v_out, int64_t n)
{
	if (n <= 0) return 0;
#ifdef SSG_EMU
	std::vector<int64_t> ix((size_t)n);
	for (int64_t i = 0; i < n; ++i) ix[(size_t)i] = i;
	std::stable_sort(ix.begin(), ix.end(), [&](int64_t a, int64_t b) { return k_in[a] > k_in[b]; });
	for (int64_t i = 0; i < n; ++i) { k_out[i] = k_in[ix[(size_t)i]]; v_out[i] = v_in[ix[(size_t)i]]; }
	return 0;
#else
	return prim_run("rocprim radix_sort_pairs_desc", [&](void *tmp, size_t &tb, hipStream_t s) { return rocprim::radix_sort_pairs_desc(tmp, tb, k_in, k_out, v_in, v_out, (size_t)n, 0u, (unsigned)(8 * sizeof(K)), s); });
#endif
}

/* inclusive running maximum: out[i] = max(in[0 .. i]) */
template <class T> static inline int prim_scan_max(const T *in, T *out, int64_t n)
{
	if (n <= 0) return 0;
#ifdef SSG_EMU
	T m = in[0];
	for (int64_t i = 0; i < n; ++i) { m = in[i] > m ? in[i] : m; out[i] = m; }
	return 0;
#else
	return prim_run("rocprim inclusive_scan", [&](void *tmp, size_t &tb, hipStream_t s) { return rocprim::inclusive_scan(tmp, tb, in, out, (size_t)n, prim_max<T>(), s); });
#endif
}

/* exclusive prefix sums of n counts, widened before they are added: out[i] = in[0] + .. + in[i - 1] for i < n */
template <class TI, class TO> static inline int prim_exsum(const TI *in, TO *out, int64_t n)
{
	if (n <= 0) return 0;
#ifdef SSG_EMU
	TO t = 0;
	for (int64_t i = 0; i < n; ++i) { out[i] = t; t += (TO)in[i]; }
	return 0;
#else
	rocprim::transform_iterator<const TI*, prim_widen<TI, TO>, TO> it(in, prim_widen<TI, TO>());
	return prim_run("rocprim exclusive_scan", [&](void *tmp, size_t &tb, hipStream_t s) { return rocprim::exclusive_scan(tmp, tb, it, out, (TO)0, (size_t)n, rocprim::plus<TO>(), s); });
#endif
}

/* number of non-zero flags, on the host (a template like the others, so that only a unit that calls it carries rocPRIM's reduce kernels) */
template <class F> static inline int prim_count_flags(const F *flag, int64_t n, uint64_t *count)
{
	*count = 0;
	if (n <= 0) return 0;
#ifdef SSG_EMU
	uint64_t c = 0; for (int64_t i = 0; i < n; ++i) c += flag[i] != 0;
	*count = c; return 0;
#else
	dbuf<uint64_t> d_out(1);
	if (!d_out.ok()) { ssg_err_msg = "device allocation failed: flag count"; return SSG_ENOMEM; }
	rocprim::transform_iterator<const F*, prim_widen<F, uint64_t>, uint64_t> it(flag, prim_widen<F, uint64_t>());
	const int rc = prim_run("rocprim reduce", [&](void *tmp, size_t &tb, hipStream_t s) { return rocprim::reduce(tmp, tb, it, d_out.p, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), s); });
	return rc ? rc : d_out.down(count, 1);
#endif
}

/* out[] = in[i] for every i with flag[i] != 0, in order; their number on the host */
template <class T> static inline int prim_select(const T *in, const uint8_t *flag, int64_t n, T *out, uint64_t *n_out)
{
	*n_out = 0;
	if (n <= 0) return 0;
#ifdef SSG_EMU
	uint64_t c = 0;
	for (int64_t i = 0; i < n; ++i) if (flag[i]) out[c++] = in[i];
	*n_out = c; return 0;
#else
	dbuf<uint64_t> d_cnt(1);
	if (!d_cnt.ok()) { ssg_err_msg = "device allocation failed: select count"; return SSG_ENOMEM; }
	const int rc = prim_run("rocprim select", [&](void *tmp, size_t &tb, hipStream_t s) { return rocprim::select(tmp, tb, in, flag, out, d_cnt.p, (size_t)n, s); });
	return rc ? rc : d_cnt.down(n_out, 1);
#endif
}
#endif
