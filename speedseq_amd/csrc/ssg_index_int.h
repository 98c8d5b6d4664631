/*
 * ssg_index_int.h -- the FM-index object shared by the translation units of libssgpu
 * (ssgpu_core.cpp: load / use; ssg_index_build.cpp: construction, upstream `bwa index`).
 */
#ifndef SSG_INDEX_INT_H
#define SSG_INDEX_INT_H
#include <vector>
#include <string>
#include <mutex>
#include <string.h>
#include "ssg_types.h"

struct ssg_hole_t { int64_t offset; int32_t len; char amb; };   /* upstream bntamb1_t (.amb) */

struct ssg_index {
	ssg_index_view_t v;
	/* owned device arrays (NULL when borrowed from the caller, ssg_index_from_device) */
	uint32_t *bwt; uint64_t *sa; uint8_t *pac; int64_t *ctg_off; int32_t *ctg_len;
	/* intervals of every pattern of 1..ktab_k bases (k_smem2.h), handed to the seeding kernel as arguments of its own -- the by-value view every
	 * kernel takes stays as small as it is */
	uint64_t *ktab; int ktab_k;
	uint64_t bwt_words;                     /* u32 words of the .bwt body (0 when borrowed) */
	bool raw_alloc;                         /* bwt/sa/pac came from rt_malloc_raw (index builder) */
	std::vector<std::string> names, annos;  /* .ann: name and FASTA comment ("" = upstream's "(null)") */
	std::vector<int32_t> n_ambs;            /* .ann: holes per contig */
	std::vector<ssg_hole_t> holes;          /* .amb */
	std::vector<int64_t> h_off; std::vector<int32_t> h_len;
	/* the contig names in HBM, for the kernel that writes SA / XA strings (k_bam.h); made by the first call that needs them (ssg_bam.cpp), dropped by ssg_index_set_names */
	std::mutex names_mu; char *d_names; int32_t *d_name_off;
	ssg_index() : bwt(0), sa(0), pac(0), ctg_off(0), ctg_len(0), ktab(0), ktab_k(0), bwt_words(0), raw_alloc(false), d_names(0), d_name_off(0) { memset(&v, 0, sizeof(v)); }
};
/* ssg_seed.cpp: the product's seeding kernels (k_smem2.h), the table of short-pattern intervals (every constructor of an index ends with
 * ssg_index_build_ktab) and the self-check of the denser suffix-array copy (SSG_SA_VERIFY) */
extern "C" int ssg_index_build_ktab(ssg_index *ix);
extern "C" int ssg_seed_smem2(const ssg_index *idx, const ssg_mem_opt_t *opt, int n_reads, const uint8_t *d_seq, const int64_t *d_off, int max_len, int cap,
                              ssg_intv_t *d_intv, int32_t *d_n, unsigned long long *n_extend, unsigned int max_ext, uint32_t *d_n_ext_read);
/* (for the test entry ssg_dbg_smem_ext: d_paths = 4 zeroed device counters -- reads the wave kernel resumed in pass 1 at x > 0, resumed in pass 2, started again because the
 * third pass was unfinished, took up in pass 1 at the read's start) */
extern "C" int ssg_seed_smem2_paths(const ssg_index *idx, const ssg_mem_opt_t *opt, int n_reads, const uint8_t *d_seq, const int64_t *d_off, int max_len, int cap,
                                    ssg_intv_t *d_intv, int32_t *d_n, unsigned long long *n_extend, unsigned int max_ext, unsigned int *d_paths);
/* (for the test entry ssg_dbg_extend_coop: the forms of one extension per item, cd[t] = base | is_back << 2; device buffers, d_lean4 / d_coop4 of 4 n entries) */
extern "C" int ssg_seed_dbg_extend_coop(const ssg_index *idx, int n, const ssg_intv_t *d_in, const uint8_t *d_cd, ssg_intv_t *d_lean, ssg_intv_t *d_coop,
                                        ssg_intv_t *d_lean4, ssg_intv_t *d_coop4);
extern "C" int ssg_sa_verify(const ssg_index *ix, int new_intv, const uint64_t *d_sa_new, long n_new);
/* ssg_bgzf_frame.cpp: the launchers of the CRC-32 and framing kernels (k_bgzf_frame.h), queued on the calling thread's stream; device buffers */
extern "C" int ssg_crc32_ranges_dev(const uint8_t *d_data, const uint64_t *d_cut, long n, uint32_t *d_crc);
extern "C" int ssg_bgzf_frame_dev(const uint8_t *d_tmp, uint32_t tmp_stride, const uint64_t *d_cut, const uint64_t *d_moff, const uint32_t *d_crc, long n_blocks, uint8_t *d_dense);
/* ssg_bgzf_deep.cpp: the deflate kernel of levels 7-9 (k_bgzf_deep.h) in the place of ssg_k_bgzf_deflate: the search depth of a level (0: not its level), the bytes of
 * link scratch for nb blocks, and the launcher, queued on the calling thread's stream; device buffers */
extern "C" int ssg_bgzf_deep_depth(int level);
extern "C" size_t ssg_bgzf_deep_scratch(long nb);
extern "C" int ssg_bgzf_deflate_deep_dev(const uint8_t *d_pay, const uint64_t *d_cut, long nb, uint8_t *d_tmp, uint32_t *d_sym, uint32_t *d_size, uint16_t *d_prev, int depth);
/* ssg_bgzf_inflate.cpp: the walk of the members' headers on the host (rng[2b], rng[2b + 1]: member b's deflate stream in members[]; out_off[]: the prefix sum of
 * the ISIZEs; SSG_EINVAL with `who' and the member in ssg_last_error()), and the launcher of the inflate and CRC-32 kernels for at most 4096 members, queued on
 * the calling thread's stream; device buffers */
extern "C" int ssg_bgzf_walk_members(const char *who, const uint8_t *members, const uint64_t *moff, long n_blocks, uint64_t *rng, uint64_t *out_off);
extern "C" int ssg_bgzf_inflate_dev(const uint8_t *d_in, const uint64_t *d_rng, const uint64_t *d_ooff, long nb, uint8_t *d_out, int32_t *d_st, uint32_t *d_crc);
/* ssg_rec_gather.cpp: the launcher of the gather kernel (k_rec_gather.h), queued on the calling thread's stream: bytes v0 .. v1 of the store's sorted stream to
 * d_out[0 .. v1 - v0), a device buffer with room for v1 - v0 bytes rounded up to 16 */
struct ssg_recs;
extern "C" int ssg_recs_gather_dev(const ssg_recs *r, uint64_t v0, uint64_t v1, uint8_t *d_out);

/* Layout fingerprint of the declarations the translation units of libssgpu share (and that kernels take by value).  Every unit defines
 * one with SSG_ABI_FP_DEFINE(<unit>); ssg_abi_selfcheck() (ssgpu_core.cpp, run before the first index is made) compares them and refuses
 * to go on when two units were compiled against different declarations -- an object left over from before a header changed would
 * otherwise read another unit's structures at the wrong offsets without any diagnostic. */
#include <stddef.h>
struct ssg_abi_fp_t { uint32_t v[20]; };
#ifdef __clang__
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
#else
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Winvalid-offsetof"
#endif
static inline ssg_abi_fp_t ssg_abi_fp_make()
{
	ssg_abi_fp_t f = {{ (uint32_t)sizeof(ssg_index_view_t), (uint32_t)sizeof(ssg_mem_opt_t), (uint32_t)sizeof(ssg_index), (uint32_t)sizeof(ssg_intv_t),
		(uint32_t)offsetof(ssg_index_view_t, primary), (uint32_t)offsetof(ssg_index_view_t, L2), (uint32_t)offsetof(ssg_index_view_t, l_pac), (uint32_t)offsetof(ssg_index_view_t, sa_intv),
		(uint32_t)offsetof(ssg_mem_opt_t, min_seed_len), (uint32_t)offsetof(ssg_mem_opt_t, split_width), (uint32_t)offsetof(ssg_mem_opt_t, max_mem_intv), (uint32_t)offsetof(ssg_mem_opt_t, split_factor),
		(uint32_t)offsetof(ssg_mem_opt_t, mat), (uint32_t)offsetof(ssg_index, bwt), (uint32_t)offsetof(ssg_index, ktab), (uint32_t)offsetof(ssg_index, bwt_words),
		(uint32_t)offsetof(ssg_index, names), (uint32_t)sizeof(ssg_seed_t), (uint32_t)sizeof(ssg_alnreg_t), (uint32_t)sizeof(ssg_aln_t) }};
	return f;
}
#ifdef __clang__
#pragma clang diagnostic pop
#else
#pragma GCC diagnostic pop
#endif
#define SSG_ABI_FP_DEFINE(unit) extern "C" void ssg_abi_fp_##unit(ssg_abi_fp_t *out) { *out = ssg_abi_fp_make(); }
extern "C" int ssg_abi_selfcheck(void);   /* 0, or SSG_EINVAL with the differing unit / field in ssg_last_error() */
#endif
