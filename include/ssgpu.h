/*
 * ssgpu.h -- C ABI of libssgpu.so, the MI355X-native `speedseq align` hot path
 * (BWA-MEM seed-and-extend + SAMBLASTER duplicate/discordant/splitter marking).
 *
 * This is the drop-in boundary below the reference's process-level plugin surface
 * (/root/reference/bin/speedseq.config:13-14 names the `bwa` and `samblaster` executables;
 * /root/reference/bin/speedseq:438-439 is the command line they must honour).  The reference's
 * src/bwa and src/samblaster are empty submodules, so each entry point cites the upstream
 * library function whose role it takes (upstream bwamem.h / ksw.h / bwt.h, SURVEY.md 8b last row)
 * and the SURVEY.md 8a row it implements.  Plain pointers and sizes only; the caller owns every
 * buffer it passes; all functions return 0 on success or a negative SSG_E* code; no globals
 * besides the HIP runtime's own state.  Host buffers are copied to HBM by the library; `*_dev`
 * variants take device pointers.
 */
#ifndef SSGPU_H
#define SSGPU_H
#include <stdint.h>
#include <stddef.h>
#include "../speedseq_amd/csrc/ssg_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SSG_OK         0
#define SSG_ENODEV   (-19)  /* no MI355X / HIP device: the library never falls back to the CPU */
#define SSG_ENOMEM   (-12)
#define SSG_EINVAL   (-22)
#define SSG_EIO      (-5)
#define SSG_EOVERFLOW (-75) /* an on-device capacity was exceeded; nothing was silently dropped */
#define SSG_EALIGN   (-71)  /* ssg_recs_scan: a BGZF block that does not start at a record -- a property of the file, callers fall back on it */
#define SSG_ERANGE   (-34)   /* ssg_b2f_push: more eligible records share one name hash than the pairing kernel takes -- a property of the input, callers fall back on it */
#define SSG_EHIP     (-1000)

const char *ssg_version(void);
const char *ssg_backend(void);            /* "hip:gfx950" (or "emu" for the CPU test build) */
int ssg_device_count(void);
int ssg_set_device(int dev);
/* Several calls in flight on one device: a thread that calls ssg_set_lane(k), 0 < k < 8, runs everything it does afterwards on stream k of
 * its device with an arena of its own, so that one thread's uploads and downloads overlap another's kernels.  Lane 0 (the default)
 * is the default stream: one call at a time per device.  One thread per (device, lane); an index loaded on any lane serves all. */
int ssg_set_lane(int lane);
const char *ssg_last_error(void);

/* upstream mem_opt_init() (bwamem.c) -- SURVEY 8a defaults, Appendix B */
void ssg_mem_opt_init(ssg_mem_opt_t *opt);

/* ---- FM-index (upstream bwa_idx_load / bwa_idx_destroy, bwa.c; row a1) ---- */
typedef struct ssg_index ssg_index_t;
int ssg_index_load(const char *prefix, ssg_index_t **out);      /* reads prefix.{bwt,sa,pac,ann} into HBM */
/* The denser copy of the suffix array this library locates seeds through (every 4th row instead of the file's every 32nd) costs one
 * LF walk over the whole text when the index is loaded; it pays for itself after some tens of millions of reads.  A caller that does
 * not know how much input is coming loads with the file's density (defer_dense_sa != 0: same results, seed location walks further)
 * and calls ssg_index_densify() once the input has proved long -- between device calls, never while one runs on this index. */
int ssg_index_load2(const char *prefix, int defer_dense_sa, ssg_index_t **out);
int ssg_index_densify(ssg_index_t *idx);                         /* no-op when the index already is as dense as SSG_SA_INTV asks */
int ssg_index_densify_to(ssg_index_t *idx, int intv);             /* the same to every intv-th row (power of two below the current interval, else a no-op); the walk costs the same at any density */
/* (All index constructors fill the HBM copy of the suffix-array samples to every 4th row -- SSG_SA_INTV overrides -- with
 *  upstream's bwt_sa walk: 2 bytes of HBM per reference base, same locations, ~6x less work per located seed.) */
int ssg_index_from_arrays(const uint32_t *bwt, uint64_t bwt_words, uint64_t primary, const uint64_t L2[5],
                          const uint64_t *sa, uint64_t n_sa, int sa_intv,
                          const uint8_t *pac, int64_t l_pac,
                          int n_ctg, const int64_t *ctg_off, const int32_t *ctg_len, ssg_index_t **out);
/* upstream `bwa index` (bwtindex.c bwa_idx_build -> bntseq.c bns_fasta2bntseq + bwt_pac2bwt + bwt_bwtupdate_core + bwt_cal_sa;
 * the reference runs it at bin/speedseq:386-391 when any of the five index files is missing).  The suffix array
 * of fwd || revcomp(fwd) is built in HBM with 64-bit positions (no 2^31 / 2^32 limit); non-ACGT bases become lrand48() & 3
 * after srand48(11) and are recorded as .amb holes, as upstream does.  `fasta` may be gzip-compressed. */
int ssg_index_build_fasta(const char *fasta, ssg_index_t **out);
/* same from forward-strand nt4 codes (0..3, no holes) already resident in HBM; contigs are named "1".."n" until ssg_index_set_names */
int ssg_index_build_dev(const uint8_t *d_fwd, int64_t l_pac, int n_ctg, const int64_t *ctg_off, const int32_t *ctg_len, ssg_index_t **out);
/* upstream bns_dump + bwt_dump_bwt + bwt_dump_sa: prefix.{amb,ann,pac,bwt,sa} byte-identical to `bwa index` output (.sa interval 32) */
int ssg_index_save(const ssg_index_t *idx, const char *prefix);
void ssg_index_destroy(ssg_index_t *idx);
int64_t ssg_index_l_pac(const ssg_index_t *idx);
int ssg_index_n_ctg(const ssg_index_t *idx);

/* ---- stage-level batched entry points (host buffers) ---- */

/* upstream ksw_extend2() (ksw.c; row a7), one job per wavefront.  qbuf/tbuf hold nt4 codes. */
int ssg_extend_batch(const ssg_mem_opt_t *opt, int n_jobs, const ssg_ext_job_t *jobs,
                     const uint8_t *qbuf, size_t qbytes, const uint8_t *tbuf, size_t tbytes,
                     ssg_ext_res_t *res, uint64_t *cells);

/* upstream ksw_align2() (ksw.c; row a10), one job per wavefront. */
int ssg_align2_batch(const ssg_mem_opt_t *opt, int n_jobs, const ssg_sw_job_t *jobs,
                     const uint8_t *qbuf, size_t qbytes, const uint8_t *tbuf, size_t tbytes, ssg_kswr_t *res);

/* upstream ksw_global2() (ksw.c; row a12): score + CIGAR (ops packed len<<4|op, "MIDSH").
 * cigar: n_jobs x cap entries. */
int ssg_global_batch(const ssg_mem_opt_t *opt, int n_jobs, const ssg_glb_job_t *jobs,
                     const uint8_t *qbuf, size_t qbytes, const uint8_t *tbuf, size_t tbytes,
                     int32_t *score, int32_t *n_cigar, uint32_t *cigar, int cap);

/* upstream mem_collect_intv() (bwamem.c; rows a1-a2).  seq: concatenated nt4 codes, off[n_reads+1].
 * out_intv: n_reads x cap; out_n[r] = number of intervals (reads that overflow cap are re-run
 * internally with a larger capacity; SSG_EOVERFLOW if `cap` cannot hold a read's final list). */
int ssg_smem_batch(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_reads, const uint8_t *seq, const int64_t *off,
                   int cap, ssg_intv_t *out_intv, int32_t *out_n);

/* Seeds of a batch of reads in upstream's visiting order (mem_chain(): for every interval of mem_collect_intv, every sampled occurrence:
 * bwt_sa() + bns_intv2rid(); rows a1-a3), before chaining.  seed_off[n_reads + 1]; *seeds and *rids (bns_intv2rid per seed, < 0 = a seed
 * upstream drops) are malloc'd by the library (ssg_free). */
int ssg_seeds_batch(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_reads, const uint8_t *seq, const int64_t *off,
                    int64_t *seed_off, ssg_seed_t **seeds, int32_t **rids);

/* upstream ksw_extend2() through the LANE-per-extension kernel code the product's mem_chain2aln path runs (k_extlane.h; ssg_extend_batch
 * above goes through the wave-per-extension code): job i's target is jobs[i].tlen bases from doubled coordinate tpos[i] of the index's
 * 2-bit reference in direction dir (+1 / -1; jobs[i].toff is ignored), its query qbuf[qoff .. qoff + qlen).  qcap selects the kernel
 * instance (72 / 136 / 256 columns of LDS per lane; every qlen must fit).  Limits of the packed DP cells: h0 + qlen * a < 8191. */
int ssg_extend_lane_batch(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_jobs, const ssg_ext_job_t *jobs, const int64_t *tpos, int dir,
                          const uint8_t *qbuf, size_t qbytes, int qcap, ssg_ext_res_t *res, uint64_t *cells);

/* upstream ksw_align2() as mate rescue runs it in the product path (row a10; k_mswlane.h): the forward pass of every job by the LANE kernel
 * (`lanes` = 1, 2 or 4 lanes per job, strips of 8 target rows in registers, strip boundaries in LDS), the reverse pass (KSW_XSTART) by the
 * wave code; a job the lane kernel does not take (KSW_XSTOP, a window above 8192 rows, scores beyond the packed cells: a > 15, b > 16,
 * qlen * a > 8190) goes through the wave code entirely.  Job i's target is jobs[i].tlen bases from doubled coordinate
 * tpos[i] of the index's 2-bit reference (jobs[i].toff is ignored), its query qbuf[qoff .. qoff + qlen).  from_lane[i] (may be NULL) = 1 when
 * the forward pass of job i came from the lane kernel. */
int ssg_align2_lane_batch(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_jobs, const ssg_sw_job_t *jobs, const int64_t *tpos,
                          const uint8_t *qbuf, size_t qbytes, int lanes, ssg_kswr_t *res, int32_t *from_lane);

/* Test entries of the seeding kernels (csrc/k_smem2.h).
 *   ssg_dbg_extend_coop  one upstream bwt_extend per item, followed base base[t] (0 .. 3) and direction is_back[t] (0 / 1) on interval in[t] (x0, x1, x2; info is
 *                        ignored), once by ssg_bwt_extend1_lean, the lane kernel's form (out_lean), and once by s2_extend_coop, the form of the wave-per-read
 *                        kernel's chains, whose rank work 16 lanes share (out_coop): the two must be equal in x0, x1, x2 and info.  out_lean4 / out_coop4 (4 n
 *                        entries): entry 4 t + g is the interval of item (t + g) mod n extended by item t's base in item t's direction, by ssg_bwt_extend1_lean and by
 *                        s2_extend_coop4, the form of the kernel's short backward rows, which does four intervals at once; equal again.  Validated first,
 *                        SSG_EINVAL otherwise: the rank queries of either direction inside the text (x0 + x2 and x1 + x2 <= text length + 1).
 *   ssg_dbg_smem_ext     ssg_smem_batch through the seeding stage's two kernels alone, with what the stage reports to the step's summary: *n_extend = the
 *                        bwt_extend calls of upstream mem_collect_intv on these reads, whichever kernel took a read and however often it started on it.  The
 *                        lists are unsorted (the stage sorts them afterwards); a list longer than cap is SSG_EOVERFLOW.  SSG_SMEM_MAX_EXT / SSG_SMEM_MAX_ROW /
 *                        SSG_KTAB_K act as in the pipeline.  paths[4]: the reads the wave-per-read kernel took up and how -- [0] resumed in pass 1 where the lane kernel's
 *                        unfinished call began, at x > 0; [1] resumed in pass 2; [2] started again because the lane kernel had not finished the third pass; [3] taken up
 *                        in pass 1 at the read's start. */
int ssg_dbg_extend_coop(const ssg_index_t *idx, int n, const ssg_intv_t *in, const uint8_t *base, const uint8_t *is_back, ssg_intv_t *out_lean, ssg_intv_t *out_coop,
                        ssg_intv_t *out_lean4, ssg_intv_t *out_coop4);
int ssg_dbg_smem_ext(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_reads, const uint8_t *seq, const int64_t *off, int cap, ssg_intv_t *out_intv, int32_t *out_n,
                     uint64_t *n_extend, uint32_t paths[4]);

/* Test hook for the chaining kernels' weight sort (csrc/k_chainw.h wv_introsort_whi; upstream ks_introsort over chain weights, bwamem.c mem_chain_flt's
 * ks_introsort(mem_flt, ...) with its unstable tie order): sorts n <= 5120 words (w << 32 | id) by w, descending, once by the whole wave (out_wave) and
 * once by one lane running the textbook loops (out_lane); the two must be equal word for word. */
int ssg_dbg_chain_sort(const int64_t *keys, int n, int64_t *out_lane, int64_t *out_wave);

/* Test entry of the chaining stage (rows a4-a5: upstream mem_chain with test_and_merge, mem_chain_weight, mem_chain_flt, frac_rep): the stage on seeds and
 * intervals given by the caller instead of the seeding stage's, through the one host function stage 1 of the pipeline runs -- the class split by seed count, every
 * kernel form under the SSG_CHAIN_* switches, the second pass on klib's B-tree.  The kernels read l_pac and n_ctg of the index and nothing else, so no index is needed.
 *   read_len[n_reads]; read r's seeds are seeds[seed_off[r] .. seed_off[r + 1]) in upstream's visiting order (rbeg, qbeg, len are read; score and next are ignored)
 *   with their contigs rids[] (< 0: a seed upstream drops); its intervals intv[intv_off[r] .. intv_off[r + 1]) (info and x2 are read), the source of frac_rep.
 * Validated first, SSG_EINVAL otherwise: 1 <= l_pac < 2^33, n_ctg >= 1, offsets from 0 and monotone, 1 <= read_len <= 310, 0 <= qbeg, 1 <= len, qbeg + len <= read_len,
 * 0 <= rbeg, rbeg + len <= 2 l_pac, rid < n_ctg, intervals sorted by start with 0 <= start < end <= read_len.
 * Out: chain_off[n_reads + 1]; *chains (malloc'd, ssg_free) the chains that survive the filter, in the stage's final order: pos, rid, n, w, kept, frac_rep as the
 * kernels leave them, first_seed = where the chain's n seed indices begin in *chain_seeds (malloc'd, ssg_free; indices count from the read's first seed), the other
 * fields 0; form[r] (may be NULL) = the kernel form that took read r, SSG_CHAIN_FORM_TREE added when the read was chained again on the tree. */
#define SSG_CHAIN_FORM_LANE     0   /* ssg_k_chain: one lane per read on global memory */
#define SSG_CHAIN_FORM_LDS16    1   /* ssg_k_chain_lds<16 | 32 | 64> */
#define SSG_CHAIN_FORM_LDS32    2
#define SSG_CHAIN_FORM_LDS64    3
#define SSG_CHAIN_FORM_WAVE256  4   /* ssg_k_chain_wave<256 | 512 | 1024 | 2048 | 5120> */
#define SSG_CHAIN_FORM_WAVE512  5
#define SSG_CHAIN_FORM_WAVE1024 6
#define SSG_CHAIN_FORM_WAVE2048 7
#define SSG_CHAIN_FORM_WAVE5120 8
#define SSG_CHAIN_FORM_TREE  0x10
int ssg_dbg_chain(const ssg_mem_opt_t *opt, int64_t l_pac, int n_ctg, int n_reads, const int32_t *read_len, const int64_t *seed_off, const ssg_seed_t *seeds, const int32_t *rids,
                  const int64_t *intv_off, const ssg_intv_t *intv, int64_t *chain_off, ssg_chain_t **chains, int32_t **chain_seeds, int32_t *form);

/* Test entry of the region stage (rows a6-a8: upstream mem_chain2aln for every chain in order, then mem_sort_dedup_patch with mem_patch_reg): the stage on chains
 * given by the caller instead of the chaining stage's, through the one host function stage 1 of the pipeline runs -- the extension jobs in their column classes, the
 * lane kernel, the wave kernel for what the lane kernel leaves, every form of the containment scan and of the dedup.  Of the index the kernels read the 2-bit
 * reference, l_pac and the contig table and nothing else, so no index is needed:
 *   pac[l_pac / 4 + 1] (the .pac file's layout: base k in byte k >> 2 at bits (~k & 3) * 2), n_ctg contigs that tile [0, l_pac) in order;
 *   seq / off[n_reads + 1] the reads (codes 0 .. 4); read r's seeds are seeds[seed_off[r] .. seed_off[r + 1]) (rbeg, qbeg, len are read; the score is set to len,
 *   as bwa 0.7.12 sets it); its chains are chains[chain_off[r] .. chain_off[r + 1]) in the form ssg_dbg_chain returns, so the two entries compose: rid, n, frac_rep
 *   and first_seed are read.  first_seed is an offset into chain_seeds that runs on over ALL chains of the call (0 for the first chain of read 0, the chain
 *   before's first_seed + n after that, across reads); chain_seeds[first_seed .. first_seed + n) are the chain's seeds as indices counted from the read's first
 *   seed (0 = seeds[seed_off[r]]).
 * Validated first, SSG_EINVAL with a message otherwise: 1 <= l_pac < 2^33, offsets from 0 and monotone, 1 <= read length <= 310, codes <= 4, 0 <= qbeg, 1 <= len,
 * qbeg + len <= read length, 0 <= rbeg, rbeg + len <= 2 l_pac, every chain with n >= 1 seeds of its read, first_seed running on from the chain before, no seed in
 * two chains (so chains <= seeds per read: the capacity of a read's region list), rid the contig of the chain's first seed, every seed of a chain inside the contig
 * and strand of the chain's first seed (the window is cut to them), and the scoring limits of the pipeline (a x 2 x length + 64 < 8191, a <= 31, b <= 32,
 * 0 <= -w <= 65535).
 * Out: reg_off[n_reads + 1]; *regs (malloc'd, ssg_free) the regions as the stage leaves them, every field; route[r] (may be NULL), from what the kernels leave:
 * SSG_REG_ROUTE_WAVE when the lane kernel left read r to the wave kernel, SSG_REG_ROUTE_PATCH when its list did not come from the dedup on compact keys (a pair
 * of regions reached mem_patch_reg's test, or the list had more than 2048 regions).  SSG_EOVERFLOW as from the pipeline when a reference window exceeds 32768 bases. */
#define SSG_REG_ROUTE_WAVE  1
#define SSG_REG_ROUTE_PATCH 2
int ssg_dbg_regions(const ssg_mem_opt_t *opt, const uint8_t *pac, int64_t l_pac, int n_ctg, const int64_t *ctg_off, const int32_t *ctg_len, int n_reads, const uint8_t *seq, const int64_t *off,
                    const int64_t *seed_off, const ssg_seed_t *seeds, const int64_t *chain_off, const ssg_chain_t *chains, const int32_t *chain_seeds,
                    int64_t *reg_off, ssg_alnreg_t **regs, int32_t *route);

/* Test entries of the paired-end decision stage (rows a9, a11): the stage on region lists given by the caller instead of stage 1's, through the kernels and
 * the host code of the pipeline itself -- the form that takes a pair (lane in LDS, lane on global memory, wave) is chosen as ssg_mem_process_pairs chooses it.
 * reg_off[2 n_pairs + 1]: read r's regions are regs[reg_off[r] .. reg_off[r + 1]) (read 1 and read 2 of a pair interleaved).  The lists are validated first
 * (monotone offsets, at most 4096 regions a read, 0 <= rid < contigs, 0 <= qb < qe <= 310, 0 <= rb < re <= 2 l_pac, scores >= 0): SSG_EINVAL otherwise.
 *   ssg_dbg_pestat      mem_pestat per batch: pes receives n_batches x 4 entries.
 *   ssg_dbg_pair_final  mem_mark_primary_se, mem_pair and mem_sam_pe's decision with one insert-size model pes[4] for all pairs: regs_out receives the lists as
 *                       the stage leaves them (sorted, marked), req_off[2 n_pairs + 1] and *req (malloc'd, release with ssg_free) the requests per read,
 *                       req[].reg counted in the caller's layout.  SSG_EOVERFLOW as from the pipeline when a pair exceeds an on-device capacity. */
/*   ssg_dbg_matesw      mem_matesw (mate rescue) for all pairs with one insert-size model pes[4]: seq / read_off[2 n_pairs + 1] are the reads (codes 0 .. 4), fixed[r] != 0
 *                       says that read r's list is the output of mem_sort_dedup_patch already (NULL: none is).  The lists are laid out as the pipeline lays them out, each in
 *                       a slice with head-room (headroom < 0: the pipeline's, else that many records): out_off[2 n_pairs + 1] the slices, *regs_out (malloc'd, release with
 *                       ssg_free) their records, n_out[r] the length of read r's list after rescue, err[p] the stage's error code of pair p (0: none).  counts: [0] windows
 *                       tried, [1] windows whose alignment came from a slot, [2] pairs decided by the kernel on keys, [3] listed pairs left to ssg_k_matesw, [4] listed
 *                       pairs, [5] Smith-Waterman cells, [6] windows of the pairs left to ssg_k_matesw.
 *   ssg_dbg_matesw_last the same counts of the calling thread's last rescue stage, whoever ran it (ssg_mem_process_pairs, ssg_hotpath_dev, ssg_dbg_matesw): with
 *                       windows accumulated over the call (the counters of a pipeline call start at zero). */
int ssg_dbg_pestat(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_pairs, const int64_t *reg_off, const ssg_alnreg_t *regs,
                   const int32_t *pair_batch, int n_batches, ssg_pestat_t *pes);
void ssg_dbg_matesw_last(uint64_t counts[8]);
int ssg_dbg_matesw(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_pairs, const uint8_t *seq, const int64_t *read_off, const int64_t *reg_off, const ssg_alnreg_t *regs,
                   const uint8_t *fixed, const ssg_pestat_t pes[4], int headroom, int64_t *out_off, ssg_alnreg_t **regs_out, int32_t *n_out, int32_t *err, uint64_t counts[8]);
int ssg_dbg_pair_final(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_pairs, int64_t id0, const int64_t *reg_off, const ssg_alnreg_t *regs,
                       const ssg_pestat_t pes[4], ssg_alnreg_t *regs_out, int64_t *req_off, ssg_alnreq_t **req);

/* Test entry of the record stage (row a12: upstream mem_reg2aln -> bwa_gen_cigar2 -> ksw_global2, NM and MD): CIGAR, POS, NM and MD of requests on regions, both given
 * by the caller instead of the pairing stage's, through the one host function the pipeline's request tail runs -- the gap-free lane kernel, the lane DP in its three
 * band classes, the wave kernel for what they leave (SSG_R2A_DPLANE=0: for everything with a gap).  Of the index the kernels read the 2-bit reference, l_pac and the
 * contig table (as ssg_dbg_regions); seq / off[n_reads + 1] are the reads (codes 0 .. 4); regs[n_regs] the regions (rb, re, qb, qe, truesc, w, score, sub, csub,
 * secondary are read); req[n_req] the requests: read, reg (an index into regs; < 0: the unmapped record), kind, owner, flag, mapq.
 * Validated first, SSG_EINVAL with a message otherwise: contigs that tile [0, l_pac), offsets from 0 and monotone, codes <= 4, 1 <= read length <= 310,
 * 0 <= rb < re <= 2 l_pac, no region across l_pac, re - rb <= 32768, read and reg in range, 0 <= qb < qe <= the length of every read the region is requested for, and
 * the scoring limits of the pipeline (as ssg_dbg_regions; gap open >= 0, gap extend >= 1, open + 32769 x extend < 2^27).
 * Out: alns[n_req] the records (zeroed first: an unmapped record leaves cigar and md untouched); route[k] (may be NULL), from the lists the kernels leave:
 * SSG_R2A_ROUTE_LANE the gap-free lane kernel made the record, SSG_R2A_ROUTE_DP0 / DP1 / DP2 the lane DP of band class 0 / 1 / 2 took it, SSG_R2A_ROUTE_WAVE the
 * wave kernel made it -- a DP class with WAVE is a record the lane DP handed on; 0 for the unmapped record.  *dev_err (may be NULL) = the stage's device error code
 * (5: the direction matrix exceeds its slab, 6: more than 62 CIGAR operations, 7: an MD of 319 characters or more); when it is not 0 the call returns SSG_EOVERFLOW,
 * as the pipeline does, with alns and route filled for inspection. */
#define SSG_R2A_ROUTE_LANE 1
#define SSG_R2A_ROUTE_DP0  2
#define SSG_R2A_ROUTE_DP1  4
#define SSG_R2A_ROUTE_DP2  8
#define SSG_R2A_ROUTE_WAVE 16
int ssg_dbg_reg2aln(const ssg_mem_opt_t *opt, const uint8_t *pac, int64_t l_pac, int n_ctg, const int64_t *ctg_off, const int32_t *ctg_len, int n_reads, const uint8_t *seq, const int64_t *off,
                    int64_t n_regs, const ssg_alnreg_t *regs, int64_t n_req, const ssg_alnreq_t *req, ssg_aln_t *alns, int32_t *route, int32_t *dev_err);

/* upstream mem_align1_core() (bwamem.c; rows a1-a8) for a batch of reads: SMEM -> SAL -> chain ->
 * filter -> extend -> sort/dedup/patch.  reg_off[n_reads+1] and regs (malloc'd by the library,
 * release with ssg_free) receive each read's mem_alnreg_t list in upstream order. */
int ssg_align1_batch(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_reads, const uint8_t *seq, const int64_t *off,
                     int64_t *reg_off, ssg_alnreg_t **regs, uint64_t stats[8]);

/* ---- the whole `bwa mem` paired-end hot path for a batch of pairs ----
 * upstream mem_process_seqs() (bwamem.c): worker1 = mem_align1_core per read, mem_pestat per
 * upstream batch, worker2 = mem_sam_pe per pair (rows a1-a12).
 *   seq/off     2*n_pairs reads (read1, read2 interleaved), nt4 codes, off[2*n_pairs+1]
 *   pair_batch  upstream batch index of every pair (insert-size statistics are per batch, row a9);
 *               batches are what `bwa mem -t N` would have formed (chunk_size*N bases, even count)
 *   id0         ordinal of the first pair in the whole input (upstream n_processed>>1; feeds the
 *               tie-breaking hash of mem_mark_primary_se / mem_pair)
 *   pes0        NULL to infer insert sizes, or 4 orientation entries as from `-I`
 * The result holds, per read, the SAM records to print (main records first, then XA entries). */
typedef struct ssg_pe_result ssg_pe_result_t;
int ssg_mem_process_pairs(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_pairs, const uint8_t *seq, const int64_t *off,
                          const int32_t *pair_batch, int n_batches, int64_t id0, const ssg_pestat_t *pes0, ssg_pe_result_t **out);
/* Single-end reads (upstream mem_process_seqs without MEM_F_PE, bwamem.c: worker1 = mem_align1_core, worker2 = mem_mark_primary_se with
 * id = n_processed + i, then mem_reg2sam without a mate): n_reads reads, id0 = upstream's n_processed at the first of them.  The result
 * is read through the same accessors (req_off has n_reads + 1 entries, there is no insert-size model) and printed by ssg_sam_format_se. */
int ssg_mem_process_reads(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_reads, const uint8_t *seq, const int64_t *off, int64_t id0, ssg_pe_result_t **out);
void ssg_pe_result_free(ssg_pe_result_t *r);
/* optional warm-up: page-locks the host blocks the records of `n_calls` concurrent ssg_mem_process_pairs results of about `n_pairs`
 * pairs will land in (the first calls make them otherwise, ~0.2 s each); bin/bwa runs it next to the index load */
int ssg_pe_reserve(int n_pairs, int n_calls);
int64_t ssg_pe_n_req(const ssg_pe_result_t *r);
int ssg_pe_is_se(const ssg_pe_result_t *r);                         /* 1: made by ssg_mem_process_reads */
const int64_t *ssg_pe_req_off(const ssg_pe_result_t *r);          /* 2*n_pairs+1 offsets into req/alns */
const ssg_alnreq_t *ssg_pe_req(const ssg_pe_result_t *r);     /* kind 0 = SAM record, 1 = XA entry (owner = region) */
const ssg_aln_t *ssg_pe_alns(const ssg_pe_result_t *r);
const ssg_pestat_t *ssg_pe_pes(const ssg_pe_result_t *r);         /* n_batches x 4 (FF, FR, RF, RR) */
const uint64_t *ssg_pe_stats(const ssg_pe_result_t *r);           /* [0] seeds [1] extension cells [2] rescue cells [3] rescues [4] records */

/* upstream mem_aln2sam() (bwamem.c; row a13): SAM text for every read of the batch, in input order.
 * names/quals/comments: one C string per read (quals/comments entries may be NULL).  *sam is
 * malloc'd (release with ssg_free); sam_off[2*n_pairs+1] delimits each read's lines. */
int ssg_sam_format(const ssg_index_t *idx, const ssg_mem_opt_t *opt, const ssg_pe_result_t *res, int n_pairs,
                   const char *const *names, const uint8_t *seq, const int64_t *off, const char *const *quals, const char *const *comments,
                   const char *rg_id, char **sam, int64_t *sam_off);
int ssg_sam_format_se(const ssg_index_t *idx, const ssg_mem_opt_t *opt, const ssg_pe_result_t *res, int n_reads,
                      const char *const *names, const uint8_t *seq, const int64_t *off, const char *const *quals, const char *const *comments,
                      const char *rg_id, char **sam, int64_t *sam_off);   /* single-end results: sam_off[n_reads + 1] */
/* the same for a selection of the batch's pairs: sel[0..n_sel) are pair indices, sam_off[2*n_sel+1] */
int ssg_sam_format_sel(const ssg_index_t *idx, const ssg_mem_opt_t *opt, const ssg_pe_result_t *res, const int32_t *sel, int n_sel,
                       const char *const *names, const uint8_t *seq, const int64_t *off, const char *const *quals, const char *const *comments,
                       const char *rg_id, char **sam, int64_t *sam_off);
/* the records of ssg_sam_format's lines as BAM (what `sambamba view -S -f bam`, the next stage of the reference's pipeline at
 * /root/reference/bin/speedseq:440, makes of that text: htslib-1.3.1 sam.c:835-1028 sam_parse1, sam.c:443-473 bam_write1): block_size-prefixed
 * records of every read in input order; bam_off[2*n_pairs+1] delimits each read's records.  Used by the fused plugin path,
 * where `bwa mem` hands binary records to samblaster / sambamba instead of SAM text.  *bam is malloc'd (ssg_free). */
int ssg_bam_format(const ssg_index_t *idx, const ssg_mem_opt_t *opt, const ssg_pe_result_t *res, int n_pairs,
                   const char *const *names, const uint8_t *seq, const int64_t *off, const char *const *quals,
                   const char *rg_id, uint8_t **bam, int64_t *bam_off);
/* ---- the same path with both text ends on the device (SURVEY 2.1 K1 + K11; rows a13, f2) ----
 * upstream bseq_read / kseq_read (htslib kseq.h:189-229) + mem_process_seqs + what `sambamba view -S -f bam` makes of mem_aln2sam's lines
 * (sam.c:835-1028 sam_parse1, sam.c:443-473 bam_write1) in ONE call: the FASTQ text of 2 * n_pairs plain four-line records goes to the device as it
 * is, in n_parts pieces (the two input files, say; page-locked pieces from ssg_host_alloc travel at bus speed) -- byte rec_off[r] of their
 * concatenation is the '@' of read r (read1, read2 interleaved; the caller's line scanner found them and checked the four-line form; the
 * device checks again; a record does not straddle two pieces) -- names, nt4 codes and qualities are taken from it there, and the block_size-prefixed BAM records of all reads come back
 * in input order, with the list of the pairs whose lines can reach one of samblaster's side streams under any options.  No comments (-C) on this
 * path.  pair_batch / n_batches / id0 / pes0 as for ssg_mem_process_pairs; rg_id: RG:Z value or NULL.  SSG_EINVAL with upstream's words when the
 * two reads of a pair carry different names. */
typedef struct ssg_pe_bam ssg_pe_bam_t;
int ssg_mem_process_fastq_bam(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_pairs, const uint8_t *const *parts, const int64_t *part_bytes, int n_parts,
                              const int64_t *rec_off, const int32_t *pair_batch, int n_batches, int64_t id0, const ssg_pestat_t *pes0, const char *rg_id, ssg_pe_bam_t **out);
/* the same from parsed reads (codes, names, qualities as C strings; quals or quals[r] may be NULL): any FASTQ / FASTA the reader accepts */
int ssg_mem_process_pairs_bam(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_pairs, const uint8_t *seq, const int64_t *off,
                              const char *const *names, const char *const *quals, const int32_t *pair_batch, int n_batches, int64_t id0,
                              const ssg_pestat_t *pes0, const char *rg_id, ssg_pe_bam_t **out);
void ssg_pe_bam_free(ssg_pe_bam_t *r);
const uint8_t *ssg_pe_bam_data(const ssg_pe_bam_t *r);            /* page-locked; ssg_pe_bam_bytes() bytes */
int64_t ssg_pe_bam_bytes(const ssg_pe_bam_t *r);
int64_t ssg_pe_bam_n_rec(const ssg_pe_bam_t *r);
int64_t ssg_pe_bam_n_cand(const ssg_pe_bam_t *r);
const ssg_bam_cand_t *ssg_pe_bam_cands(const ssg_pe_bam_t *r);    /* in pair order */
const ssg_pestat_t *ssg_pe_bam_pes(const ssg_pe_bam_t *r);        /* n_batches x 4 */
const uint64_t *ssg_pe_bam_stats(const ssg_pe_bam_t *r);          /* as ssg_pe_stats */
int ssg_index_set_names(ssg_index_t *idx, int n, const char *const *names);
const char *ssg_index_name(const ssg_index_t *idx, int i);
int32_t ssg_index_len(const ssg_index_t *idx, int i);

/* ---- SAMBLASTER duplicate marking (upstream samblaster.cpp markDups; row a14) ----
 * ends: 2*n_pairs primary records (read1, read2 per pair) in input order; dup[p] = 1 when an
 * earlier pair of the same call carries the same 5'-unclipped signature (first seen wins). */
int ssg_sbl_markdup(long n_pairs, const ssg_sbl_end_t *ends, uint8_t *dup);
/* streaming form: the signature table persists in HBM between calls (first-seen-wins over the whole
 * stream, as upstream's single pass) */
typedef struct ssg_sbl_state ssg_sbl_state_t;
ssg_sbl_state_t *ssg_sbl_state_new(void);
void ssg_sbl_state_free(ssg_sbl_state_t *st);
int ssg_sbl_markdup_stream(ssg_sbl_state_t *st, long n_pairs, const ssg_sbl_end_t *ends, uint8_t *dup);

/* upstream samblaster's per-block decisions on the device (samblaster.cpp block processing; rows a14-a17): `lines` are the SAM
 * lines of n_blocks name-grouped blocks (blk_off[n_blocks+1]) as numbers; on return line_bits[i] has SSG_SBL_DUP (OR 0x400 into
 * FLAG), SSG_SBL_DISC (copy to --discordantFile), SSG_SBL_SPLIT (copy to --splitterFile with _1/_2) and mate_line[i] is the
 * line whose CIGAR / MAPQ fill MC:Z / MQ:i (-1: none).  The duplicate set persists in `st` across calls (first seen wins
 * over the whole stream); st == NULL restricts it to this call. */
#define SSG_SBL_DUP   1
#define SSG_SBL_DISC  2
#define SSG_SBL_SPLIT 4
void ssg_sbl_opt_init(ssg_sbl_opt_t *o);
int ssg_sbl_process(ssg_sbl_state_t *st, const ssg_sbl_opt_t *o, long n_blocks, const int64_t *blk_off, const ssg_sbl_line_t *lines,
                    uint8_t *line_bits, int64_t *mate_line);
/* ssg_sbl_process in two halves, for several pipelines that share ONE duplicate set (rank mode: bin/speedseq-ranks).
 * samblaster keeps the first pair of every signature in input order (GregoryFaust/samblaster samblaster.cpp, the duplicate hash set; SURVEY 8a
 * a14): a pipeline extracts the two primary ends of every block (ends[2 * n_blocks]), the process that owns the set decides them with
 * ssg_sbl_markdup_stream in input order, and the lines are classified with those verdicts (dup[n_blocks]). */
int ssg_sbl_ends(long n_blocks, const int64_t *blk_off, const ssg_sbl_line_t *lines, ssg_sbl_end_t *ends);
int ssg_sbl_classify(const ssg_sbl_opt_t *o, long n_blocks, const int64_t *blk_off, const ssg_sbl_line_t *lines, const uint8_t *dup,
                     uint8_t *line_bits, int64_t *mate_line);

/* stable device radix sort of 64-bit keys, returned as a permutation: the coordinate sort of BAM records (samtools bam_sort.c:1607-1614
 * key tid<<32 | (pos+1)<<1 | reverse; ties keep input order) for the `sambamba sort` the reference runs at bin/speedseq:427 (row f1) */
int ssg_sort_u64_perm(const uint64_t *keys, int64_t n, uint32_t *perm);

/* ---- the measured hot path with device-resident inputs (bench.py) ----
 * d_seq / d_off / d_pair_batch are DEVICE pointers; aligned + duplicate-marked records stay in HBM.
 * summary: [0] records [1] duplicate pairs [2] seeds [3] extension cells [4] rescue cells [5] rescues */
int ssg_hotpath_dev(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_pairs, int max_len, const uint8_t *d_seq, const int64_t *d_off,
                    const int32_t *d_pair_batch, int n_batches, int64_t id0, uint64_t summary[8], uint8_t *dup_host);
/* Same, and the 5'-unclipped pair signatures (n_pairs x 3 uint64 in DEVICE memory; all ones = never a duplicate) that ranks
 * exchange for exact first-seen-wins duplicate marking over a sharded input (samblaster.cpp: the signature set is global). */
int ssg_hotpath_dev_sig(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_pairs, int max_len, const uint8_t *d_seq, const int64_t *d_off,
                        const int32_t *d_pair_batch, int n_batches, int64_t id0, uint64_t summary[8], uint8_t *dup_host, uint64_t *d_sig_out);

/* The whole path incl. samblaster's classification (rows a1-a12, a14-a17).  summary[0..7] as above, [8] discordant-stream lines,
 * [9] splitter-stream lines, [10] SAM lines.  sbl == NULL = the reference's switches (--excludeDups --addMateTags, bin/speedseq:439).
 * local_dedup = 0 + d_sig_out + keep: sharded input -- the caller exchanges the signatures between ranks, then classifies the
 * records still resident in HBM with the global verdicts (d_dup: DEVICE, one byte per pair; counts: dup pairs, discordant
 * lines, splitter lines, SAM lines). */
typedef struct ssg_dev_records ssg_dev_records_t;
int ssg_hotpath_dev_ex(const ssg_index_t *idx, const ssg_mem_opt_t *opt, int n_pairs, int max_len, const uint8_t *d_seq, const int64_t *d_off,
                       const int32_t *d_pair_batch, int n_batches, int64_t id0, const ssg_sbl_opt_t *sbl, int local_dedup,
                       uint64_t summary[16], uint8_t *dup_host, uint64_t *d_sig_out, ssg_dev_records_t **keep);
int ssg_dev_records_classify(ssg_dev_records_t *r, const ssg_sbl_opt_t *sbl, const uint8_t *d_dup, uint64_t counts[4]);
/* the owner rank's side of that exchange (samblaster.cpp's set is global: the first pair of a signature in INPUT order survives): for n
 * signatures received from all ranks (DEVICE: d_sig n x 3 uint64, all ones = never a duplicate; d_ordinal = global input ordinal of the
 * pair, non-negative) d_dup[i] = 1 iff an element with the same signature and a smaller ordinal exists.  Same kernels as ssg_sbl_markdup. */
int ssg_markdup_sig_dev(long n, const uint64_t *d_sig, const int64_t *d_ordinal, uint8_t *d_dup);
void ssg_dev_records_free(ssg_dev_records_t *r);
/* for the coordinate-sorted merge across ranks (SURVEY 8e coupling 3): per SAM line of the kept records, in line order, the sort key
 * of samtools bam_sort.c:1607-1614 (tid<<32 | (pos+1)<<1 | reverse), the fixed-size device record and the side-stream bits,
 * written to DEVICE buffers of the caller (d_recs / d_bits may be NULL) */
int64_t ssg_dev_records_n_lines(const ssg_dev_records_t *r);
size_t ssg_dev_record_bytes(void);
int ssg_dev_records_export(const ssg_dev_records_t *r, uint64_t *d_keys, void *d_recs, uint8_t *d_bits);
/* the kept records as a host result (release with ssg_pe_result_free; prints through ssg_sam_format) and, per SAM line in line order
 * (ssg_dev_records_n_lines entries, HOST buffers, either may be NULL), samblaster's decisions: SSG_SBL_* bits and the mate line */
int ssg_dev_records_download(const ssg_dev_records_t *r, ssg_pe_result_t **res, uint8_t *line_bits, int64_t *mate_line);
/* test entry: samblaster's stage of the timed step (rows a14-a17) on records given by the caller -- what ssg_hotpath_dev_ex runs after alignment, through the same
 * host functions: the SAM lines of the records (FLAG as mem_aln2sam prints it, CIGAR sums), the primaries and their ends, duplicate marking (against st's set
 * when st != NULL), classification, counts and the coordinate-sort keys.  req_off[2 n_pairs + 1]: read r's requests are req[req_off[r] .. req_off[r + 1]) with
 * their records in alns at the same index (read 1 and read 2 of a pair interleaved); only SSG_REQ_MAIN requests make a line.
 * Validated first, SSG_EINVAL with a message otherwise and before any launch: --maxSplitCount <= 16, offsets from 0 and monotone, kinds, 0 <= n_cigar <= SSG_MAX_CIGAR,
 * a main request for every read, and a main one first.
 * Outputs (HOST buffers of the caller): line_off[n_pairs + 1], *n_lines; per line (room for as many as there are requests) lines, line_req, bits, mate_line, keys;
 * per pair ends[2], prim[2] (line index or -1), sig[3] (all ones = never a duplicate), dup; counts[4] as ssg_dev_records_classify. */
int ssg_dbg_sbl_records(long n_pairs, const int64_t *req_off, const ssg_alnreq_t *req, const ssg_aln_t *alns, const ssg_sbl_opt_t *o, ssg_sbl_state_t *st,
                        int64_t *line_off, int64_t *n_lines, ssg_sbl_line_t *lines, int64_t *line_req, ssg_sbl_end_t *ends, int64_t *prim, uint64_t *sig, uint8_t *dup,
                        uint8_t *bits, int64_t *mate_line, uint64_t counts[4], uint64_t *keys);

/* FM-index from arrays already resident in HBM (not copied; the caller keeps them alive) */
int ssg_index_from_device(const uint32_t *d_bwt, uint64_t primary, const uint64_t L2[5], const uint64_t *d_sa, int sa_intv,
                          const uint8_t *d_pac, int64_t l_pac, int n_ctg, const int64_t *ctg_off, const int32_t *ctg_len, ssg_index_t **out);

/* per-kernel device time of the calls made since ssg_prof_reset() (HIP events on the launch stream).
 * ssg_prof_get: returns the number of kernels; name[i] / ms[i] / launches[i] for i < min(n, cap). */
void ssg_prof_enable(int on);
void ssg_prof_reset(void);
int ssg_prof_get(int cap, const char **name, double *ms, long *launches);

void ssg_free(void *p);

/* ---- the exchange step of the path over several GPUs (SURVEY 8e coupling 3: the coordinate-sorted merge; the reference ends in ONE OUT.bam,
 * /root/reference/bin/speedseq:441,491-495) ----
 * One process per GPU (bin/speedseq-ranks); every rank's `sambamba sort` owns a stretch of the genome and receives the records of that stretch from all ranks:
 * an all-to-all of variable-size blocks, here as grouped ncclSend / ncclRecv over RCCL (every xGMI link of a device at once; no ring).  ssg_coll_init: the
 * communicator over the calling process's device; rank 0 leaves the unique id in rendezvous_dir (a directory all ranks share).  Blocks are host buffers
 * (the records are made by host stages) staged through HBM.  SSG_ENODEV when there is no device or no RCCL: the caller's other transports take over. */
typedef struct ssg_coll ssg_coll_t;
int ssg_coll_available(void);   /* 1: a device is visible and RCCL loads (the ranks tell one another before any of them enters ssg_coll_init, which is collective) */
int ssg_coll_init(int rank, int world, const char *rendezvous_dir, ssg_coll_t **out);
int ssg_coll_alltoallv(ssg_coll_t *c, const void *const *send, const uint64_t *send_bytes, void *const *recv, const uint64_t *recv_bytes);   /* block q to / from rank q */
int ssg_coll_alltoall_u64(ssg_coll_t *c, const uint64_t *send, uint64_t *recv, int k);   /* k values to / from every rank */
void ssg_coll_destroy(ssg_coll_t *c);

/* ---- BGZF on the device (row f1; htslib bgzf.c:298-342 is the format's writer in the reference) ----
 * Block b's payload is payload[cut[b] .. cut[b+1]) (<= 0xff00 bytes, as bgzf_write cuts them); SSG_EINVAL for a larger one, SSG_EOVERFLOW when out_cap
 * is too small (nothing is written behind out + out_cap), n_blocks <= 0: out_off[0] = 0 and nothing else.  Host buffers; page-locked ones
 * (ssg_host_alloc) travel at bus speed.
 * ssg_bgzf_deflate: the block's raw deflate stream (RFC 1951, one final block; stored when it would not shrink) lands at out[out_off[b] .. out_off[b+1]),
 * for a caller that frames it itself.  out_cap: the sum of the payloads + 5 per block always suffices. */
int ssg_bgzf_deflate(const uint8_t *payload, const uint64_t *cut, long n_blocks, uint8_t *out, uint64_t out_cap, uint64_t *out_off);
/* ssg_bgzf_compress: ssg_bgzf_deflate plus framing (bgzf.c:298-342): out[out_off[b] .. out_off[b+1]) is the complete BGZF member of block b -- the 18-byte
 * header with BSIZE, the same deflate stream, CRC-32 and ISIZE of the payload, all made on the device; concatenated they are a BGZF file's body.  A block
 * without payload becomes the 28-byte end-of-file marker: a caller ends a file by appending one.  crc (may be NULL) receives the payloads' CRC-32. */
int ssg_bgzf_compress(const uint8_t *payload, const uint64_t *cut, long n_blocks, uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint32_t *crc);
/* The forms with a deflate level (zlib's scale; ssg_bgzf_compress_recs_level: below, with the record store).  1..6: the calls above, byte for byte -- the device has
 * one parse below 7.  7, 8, 9: a chained match finder (csrc/k_bgzf_deep.h) that looks at up to 8 / 32 / 128 earlier positions of the hash, nearest first, where the
 * parse above looks at six: smaller streams, more kernel time; the same contract (any inflate gives back the payload, a block that would not shrink is stored).
 * SSG_EINVAL for level 0 (the device writes no stored-only file) and for anything outside 1..9. */
int ssg_bgzf_deflate_level(const uint8_t *payload, const uint64_t *cut, long n_blocks, uint8_t *out, uint64_t out_cap, uint64_t *out_off, int level);
int ssg_bgzf_compress_level(const uint8_t *payload, const uint64_t *cut, long n_blocks, uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint32_t *crc, int level);
/* an out_cap that always suffices for ssg_bgzf_compress: payload + 31 per block (5 of the stored form, 26 of header and trailer; bgzf.c:298-342) */
uint64_t ssg_bgzf_bound(uint64_t payload_bytes, long n_blocks);
/* CRC-32 (zlib's, the one of a BGZF member's trailer, bgzf.c:298-342) of n byte ranges data[cut[i] .. cut[i+1]) of any length, on the device; host buffers.
 * One wavefront per range: made for many ranges of BGZF-block size; a single range of many megabytes keeps one wavefront of the device busy. */
int ssg_crc32_batch(const uint8_t *data, const uint64_t *cut, long n, uint32_t *crc);
/* ssg_bgzf_inflate: the inverse of ssg_bgzf_compress (the reader in the reference: htslib bgzf.c, bgzf_read_block / check_header / inflate_block; the stream:
 * RFC 1951, judged as zlib's inflate judges it).  members[moff[b] .. moff[b+1]) is one complete BGZF member -- header with the BC subfield, deflate stream of any
 * block types, CRC-32, ISIZE; concatenated they are a BGZF file's body.  The host walks the headers: SSG_EINVAL, with the member's index in ssg_last_error(), for
 * a member that is no gzip member with FEXTRA, has no BC subfield, a BSIZE + 1 other than its span, a span below 28 bytes or an ISIZE above 65536.  out_off[]
 * becomes the prefix sum of the ISIZEs (out_off[0] = 0); SSG_EOVERFLOW when out_off[n_blocks] > out_cap (nothing is written behind out + out_cap);
 * n_blocks <= 0: out_off[0] = 0 and nothing else.  The device inflates a wavefront per member to out[out_off[b] .. out_off[b+1]) and checksums the output.
 * status (may be NULL): 0 good; 1 malformed stream; 2 the stream's output is not ISIZE bytes (shorter, or more to come); 3 CRC-32 mismatch.  Returns 0 when
 * every member is good, SSG_EIO when one is not: status[] is complete then, the good members' output intact, a bad member's range unspecified (and only that
 * range touched).  Bytes behind the final block's end are no error; an empty member (the end-of-file marker) is good and produces nothing.  Host buffers. */
int ssg_bgzf_inflate(const uint8_t *members, const uint64_t *moff, long n_blocks, uint8_t *out, uint64_t out_cap, uint64_t *out_off, int32_t *status);
/* ---- the records of a sort in HBM, and their sorted stream gathered there (row f1; stands for bgzf_write's copy of a record into the block buffer, htslib
 * bgzf.c) ----
 * A device mirror of the chunks `sambamba sort` holds its input in.  A record's location is (chunk << 40 | offset of its block_size word), the encoding the sort
 * keeps.  All entry points: SSG_ENODEV without a device; SSG_EINVAL from a thread that drives another device than the store's.
 * ssg_recs_create: a store on the calling thread's device that will hold at most cap_bytes of chunks; nothing is allocated yet.
 * ssg_recs_append: uploads one chunk (a device allocation of its own) and returns its id; SSG_ENOMEM when the sum of the chunks would pass cap_bytes or the
 *   device has no room -- the store is unchanged and usable.  One thread appends.
 * ssg_recs_order: declares the sorted stream: record i lies at loc[i] and occupies bytes cum[i] .. cum[i+1] of it (cum[0] = 0, non-decreasing; n >= 0).  Every
 *   location and length is checked against the chunks here (SSG_EINVAL with the record in ssg_last_error()): the kernel has no bounds of its own.  Afterwards
 *   the store is read-only; ssg_recs_gather and ssg_bgzf_compress_recs may be called from several threads at once, each on a lane of its own (ssg_set_lane).
 * ssg_recs_gather: stream bytes v0 .. v1 into a host buffer: the kernel with nothing around it (tests, debugging).  SSG_EINVAL for v0 > v1 or v1 > cum[n];
 *   v0 == v1 writes nothing.
 * ssg_bgzf_compress_recs: ssg_bgzf_compress of the stream bytes cut[0] .. cut[n_blocks] (cut[]: absolute stream offsets) without the payload ever being in host
 *   memory: the same members, byte for byte, the same errors. */
typedef struct ssg_recs ssg_recs_t;
int ssg_recs_create(uint64_t cap_bytes, ssg_recs_t **out);
int ssg_recs_append(ssg_recs_t *r, const uint8_t *bytes, uint64_t len, uint32_t *chunk_id);
int ssg_recs_order(ssg_recs_t *r, const uint64_t *loc, const uint64_t *cum, int64_t n);
int ssg_recs_gather(ssg_recs_t *r, uint64_t v0, uint64_t v1, uint8_t *out);
int ssg_bgzf_compress_recs(ssg_recs_t *r, const uint64_t *cut, long n_blocks, uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint32_t *crc);
int ssg_bgzf_compress_recs_level(ssg_recs_t *r, const uint64_t *cut, long n_blocks, uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint32_t *crc, int level);   /* ssg_bgzf_compress_level's levels */
void ssg_recs_free(ssg_recs_t *r);
/* ---- BAM read into the store: members inflated there, their records found there (row f1; the reader in the reference: bgzf_read_block and bam_read1, htslib) ----
 * ssg_recs_append_bgzf: ssg_bgzf_inflate whose output becomes a new chunk of the store instead of a host buffer: the same walk of the headers on the host, the
 *   same SSG_EINVAL cases, the same status[] and SSG_EIO, out_off[] the prefix sum of the ISIZEs.  The chunk holds out_off[n_blocks] bytes (plus the store's
 *   16 bytes of slack) and is never copied to the host; *chunk_id receives its id.  The capacity rule is ssg_recs_append's (SSG_ENOMEM, store unchanged and
 *   usable).  A bad member (SSG_EINVAL, SSG_EIO) leaves the store as it was: no chunk, the capacity unchanged.  n_blocks <= 0: out_off[0] = 0, no chunk.
 *   Refused (SSG_EINVAL) while an order is declared, as ssg_recs_append.
 * ssg_recs_scan: the records of a chunk.  The chunk's bytes first .. hint[n_hints] are one stream of BAM records (block_size word, block_size bytes, ...).
 *   hint[0 .. n_hints] (n_hints + 1 values, ascending, hint[n_hints] <= the chunk's length, first <= hint[n_hints]) are offsets at which a record is expected to
 *   begin -- the members' out_off[]: every mainstream writer starts a BGZF block at a record (htslib's bgzf_flush_try) -- and the intervals between them are
 *   walked side by side on the device; what lies before `first' (a header's bytes) is skipped.  Per record, in stream order: loc[i] = chunk_id << 40 | offset of
 *   its block_size word (the store's encoding); key[i] = the coordinate key of `sambamba sort' (bam1_lt: tid << 32 | (pos + 1) << 1 | reverse, tid = -1 as it
 *   comes); ent[i] = tid, pos, end (bam_endpos: pos + 1 for an unmapped record or one without CIGAR, else pos + the lengths of its M, D, N, = and X
 *   operations), flag, len = 4 + block_size, pad = 0.  loc / key / ent: host arrays of `cap' elements.  Returns
 *     0              *n_rec records returned;
 *     SSG_EOVERFLOW  cap < *n_rec: *n_rec is set, nothing is written to loc / key / ent (length of the stream / 36 always suffices as cap);
 *     SSG_EIO        a malformed stream, its offset in ssg_last_error(): a block_size below 32, a record that runs past hint[n_hints], or a record whose
 *                    l_qname + 4 n_cigar exceeds block_size - 32;
 *     SSG_EALIGN     not record-aligned at hint b (b and the offsets in ssg_last_error()): the walk that entered at hint[b] passed hint[b+1] without landing
 *                    on it.  A property of the file (a writer that splits records over blocks), not an error of the call: callers fall back on it.
 *   Nothing is valid in loc / key / ent unless 0 is returned; the store is unchanged by every outcome.  SSG_EINVAL for a chunk that does not exist or is released,
 *   or hints that do not ascend inside the chunk.
 * ssg_recs_select: ssg_recs_scan with the decision behind it, taken on the device (k_bam_select.h): the same walk, the same states, SSG_EIO, SSG_EALIGN and
 *   SSG_EINVAL with the same words in ssg_last_error() (under this entry's name).  *n_rec: the records scanned.  A record is kept when it overlaps a region and
 *   the filter program leaves 1; *n_sel: the records kept, and only their loc / key / ent come back, in stream order (host arrays of `cap' elements).
 *     reg[0 .. n_reg): 0-based, half-open (tid, beg, end), sorted by (tid, beg), disjoint and not adjacent (the caller has merged them).  A record overlaps a
 *       region when the tid is equal, pos < reg.end and rec.end > reg.beg, rec.end as in ent (bam_endpos); a record with tid < 0 overlaps nothing.
 *       n_reg == 0: no region test.
 *     prog[0 .. n_prog): a postfix program over a stack of booleans, at most SSG_FOP_MAX operations.  SSG_FOP_FLAG pushes (flag & value) != 0; SSG_FOP_EQ ..
 *       SSG_FOP_GE push `field <cmp> value' with the field named by arg (SSG_FLD_*: MAPQ, tid, mate tid, isize, l_seq, flag; signed 32-bit comparisons);
 *       SSG_FOP_AND / SSG_FOP_OR replace the two topmost values, SSG_FOP_NOT the topmost.  n_prog == 0: every record passes.
 *     SSG_EOVERFLOW  cap < *n_sel: *n_rec and *n_sel are set, nothing is written to loc / key / ent.  cap == 0 with loc, key and ent all NULL is the counting
 *                    form: it returns 0 and nothing but the two numbers.
 *     SSG_EINVAL     also for regions that are unsorted, overlap, touch, or have beg >= end, beg < 0 or tid < 0; a program of more than SSG_FOP_MAX operations, one
 *                    that underflows the stack or does not leave exactly one value, an unknown operation or field (each named in ssg_last_error()); and while
 *                    an order is declared (ssg_recs_reopen first).  The store is unchanged by every outcome.
 * ssg_recs_reopen: drops a declared order: the store takes appends again, and a later ssg_recs_order declares a new stream.
 * ssg_recs_release: frees a chunk's device memory and returns its bytes to the capacity.  The id stays taken (later chunks keep theirs); ssg_recs_order refuses
 *   a location in a released chunk with SSG_EINVAL.  Refused (SSG_EINVAL) while an order is declared: ssg_recs_reopen first. */
typedef struct { int32_t tid, pos, end; uint32_t flag, len, pad; } ssg_bam_ent_t;
int ssg_recs_append_bgzf(ssg_recs_t *r, const uint8_t *members, const uint64_t *moff, long n_blocks, uint32_t *chunk_id, uint64_t *out_off, int32_t *status);
int ssg_recs_scan(ssg_recs_t *r, uint32_t chunk_id, const uint64_t *hint, int64_t n_hints, uint64_t first, uint64_t cap, uint64_t *n_rec, uint64_t *loc, uint64_t *key, ssg_bam_ent_t *ent);
typedef struct { int32_t tid, beg, end; } ssg_bam_region_t;
typedef struct { uint8_t op, arg; uint16_t pad; int32_t value; } ssg_bam_fop_t;
#define SSG_FOP_MAX 64
enum { SSG_FOP_FLAG = 0, SSG_FOP_AND = 1, SSG_FOP_OR = 2, SSG_FOP_NOT = 3, SSG_FOP_EQ = 4, SSG_FOP_NE = 5, SSG_FOP_LT = 6, SSG_FOP_LE = 7, SSG_FOP_GT = 8, SSG_FOP_GE = 9 };
enum { SSG_FLD_MAPQ = 0, SSG_FLD_REF_ID = 1, SSG_FLD_MATE_REF_ID = 2, SSG_FLD_TLEN = 3, SSG_FLD_SEQ_LEN = 4, SSG_FLD_FLAG = 5 };
int ssg_recs_select(ssg_recs_t *r, uint32_t chunk_id, const uint64_t *hint, int64_t n_hints, uint64_t first, const ssg_bam_region_t *reg, int64_t n_reg, const ssg_bam_fop_t *prog, int n_prog,
                    uint64_t cap, uint64_t *n_rec, uint64_t *n_sel, uint64_t *loc, uint64_t *key, ssg_bam_ent_t *ent);
int ssg_recs_reopen(ssg_recs_t *r);
int ssg_recs_release(ssg_recs_t *r, uint32_t chunk_id);
/* bytes of device memory that are free / that the calling thread's device has: what a caller sizes a store from */
int ssg_device_memory(uint64_t *free_bytes, uint64_t *total_bytes);
void *ssg_host_alloc(size_t n);
void ssg_host_free(void *p);

/* ---- bamtofastq on the device (csrc/ssg_b2f.cpp, k_b2f.h): the pairs of a BAM stream as interleaved FASTQ text, byte for byte what `bamkit bamtofastq' writes ----
 * The stream is fed chunk by chunk (ssg_recs_append_bgzf, then ssg_b2f_push), files in the order given, records in file order.  A record takes part when
 * flag & 0x900 is clear, flag & 1 is set, no CIGAR operation is a hard clip and -- with a read group list -- its RG:Z is in the list (a record without one is
 * not).  The aux area is walked with the types A c C s S i I f Z H B; any other type (`d' among them), a Z / H without its NUL or a B without its five bytes
 * ends the walk, and the last RG:Z met before that counts.  Per name (the l_qname - 1 bytes, compared whole): nothing held -> the record is held; the held one
 * has the same flag & 0x40 -> the record is dropped; otherwise the pair leaves, the half with 0x40 as /1, and nothing is held.  Pairs leave in the stream order
 * of the record that completed them.  A half is `@name/1' or `@name/2', ` RG:Z:<rg>' when its own RG is not empty, `\n SEQ \n+\n QUAL \n'; flag & 0x10
 * reverses both and complements SEQ (A/T C/G M/K R/Y V/B H/D); a first quality byte 0xff gives all `I'.  With `rename' the name is a running pair number from 0.
 * ssg_b2f_create: rg[0 .. n_rg) is the read group list (n_rg == 0: no test); hash_bits in 0 .. 64 is how much of the 64-bit name hash groups the records
 *   (callers pass 64; the result does not depend on it: names are compared in full).  The object lives on the store's device and must be freed before the store.
 *   SSG_EINVAL for a NULL store, a NULL or empty id, n_rg < 0, hash_bits outside 0 .. 64.
 * ssg_b2f_push: the chunk's records are found as ssg_recs_scan finds them (the same hints, `first', SSG_EIO / SSG_EALIGN / SSG_EINVAL and words, under this
 *   entry's name) and paired with the halves carried from earlier pushes, which precede them in stream order.  The text of the pairs completed by this chunk's
 *   records goes to out[0 .. *out_len); *n_rec: the records scanned; *n_pairs: the pairs written.
 *     SSG_EIO        also a record with 32 + l_qname + 4 n_cigar + (l_seq + 1) / 2 + l_seq > block_size (its offset in ssg_last_error()): nothing is written.
 *     SSG_EOVERFLOW  *out_len > out_cap; *out_len is set.  out_cap = 2 * (chunk length + carried bytes) + 64 always suffices: a half's text is
 *                    name + 2 l_seq + 8 (+ 6 + rg) bytes, its record 36 + name + 1 + 4 n_cigar + (l_seq + 1) / 2 + l_seq (+ 4 + rg) bytes or more, and with
 *                    `rename' the number's at most 20 digits stand in for the name against the 72 bytes that two fixed parts give.
 *     SSG_ERANGE     more than SSG_B2F_RUN_MAX eligible records (carried ones included) share one hash of hash_bits bits.
 *     SSG_ENOMEM     device memory.  SSG_EINVAL also while an order is declared (ssg_recs_reopen first).
 *   On every failure the object, the store and the chunk are as before and the call may be repeated.  On success the chunk is released (ssg_recs_release), the
 *   carry -- device memory that counts against the store's capacity -- holds exactly the halves still held, and the pair number has advanced by *n_pairs.
 * ssg_b2f_waiting: the halves held and the bytes of their records (4 + block_size each). */
#define SSG_B2F_RUN_MAX 256
typedef struct ssg_b2f ssg_b2f_t;
int  ssg_b2f_create(ssg_recs_t *r, const char *const *rg, int n_rg, int rename, int hash_bits, ssg_b2f_t **out);
int  ssg_b2f_push(ssg_b2f_t *b, uint32_t chunk_id, const uint64_t *hint, int64_t n_hints, uint64_t first,
                  uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint64_t *n_rec, uint64_t *n_pairs);
int  ssg_b2f_waiting(ssg_b2f_t *b, uint64_t *n_halves, uint64_t *bytes);
void ssg_b2f_free(ssg_b2f_t *b);

/* ---- coverage on the device (csrc/ssg_depth.cpp, k_depth.h): per-position counters of a BAM stream, their sums over regions and windows, and the lines of
 * `samtools depth' (samtools 1.3.1 bam2depth.c, bedcov.c: the numbers are theirs, without the 8000 / 64000 pile caps) ----
 * The stream is fed chunk by chunk (ssg_recs_append_bgzf, then ssg_depth_push).  A record takes part when the filter program leaves 1 on it (the programs and
 * fields of ssg_recs_select), its tid >= 0 and its n_cigar > 0.  Per reference position two 32-bit counters: every position of an M, =, X, D or N operation
 * adds 1 to `span'; every position of an M, = or X operation whose base passes the quality test adds 1 to `cov'; S, I, H and P add nothing (S and I advance the
 * query).  A base passes when its quality byte, taken unsigned, is >= min_baseq (0xff passes; min_baseq == 0 passes everything); a base beyond l_seq has no byte
 * and passes, so a record with l_seq == 0 passes on every base.  Positions are 0-based reference positions everywhere.
 * ssg_depth_create: the object lives on the store's device and must be freed before the store.  SSG_EINVAL for what ssg_recs_select refuses of a program, in the
 *   same words under this entry's name, and for min_baseq outside 0 .. 255.
 * ssg_depth_begin: opens the span [beg, end) of contig tid, 0 <= beg < end <= 2^31 - 1; its counters are device memory, zeroed there.  SSG_ENOMEM with the
 *   object unchanged when they do not fit; SSG_EINVAL while a span is open.
 * ssg_depth_push: the chunk's records are found as ssg_recs_scan finds them (the same hints, `first', SSG_EIO / SSG_EALIGN / SSG_EINVAL and words, under this
 *   entry's name); every passing record with tid == the span's, pos < end and rec.end > beg (rec.end as in ssg_bam_ent_t) is added, clipped to the span.
 *   *n_rec: the records scanned; *n_used: the records added; *n_later: the passing records that matter to a later span (a greater tid, or the same tid and
 *   rec.end > the span's end: the caller keeps the chunk and pushes it again into the next span); *descents: the records whose (tid, pos) lies below their
 *   predecessor's in the chunk (a file that is not coordinate-sorted); *n_behind (may be NULL): the records, passing or not, that begin behind the span
 *   (tid < 0, a greater tid, or pos >= end): once there is one, no later chunk of a sorted stream adds to this span.  With min_baseq > 0, SSG_EIO also for a record to be added with 32 + l_qname +
 *   4 n_cigar + (l_seq + 1) / 2 + l_seq > block_size (its offset in ssg_last_error()).  The chunk is not released and the store is unchanged by every outcome;
 *   on every failure the counters are as before the call.  SSG_EINVAL also without an open span, after ssg_depth_finish, and while an order is declared.
 * ssg_depth_finish: the counters become final; ssg_depth_push is refused until the next ssg_depth_begin.  The three calls below need a finished span.
 * ssg_depth_get: the counters of positions [p0, p1) of the span to host arrays (tests, measuring).
 * ssg_depth_sums: reg[] holds n_reg pairs (beg, end) inside the span, in any order, overlapping or not; per pair out holds 2 + n_thr values: the sum of span,
 *   the sum of cov, and per threshold (at most 8) the positions with cov >= thr[k].  n_reg == 0 is allowed; SSG_EINVAL for a pair outside the span or with
 *   beg >= end.
 * ssg_depth_text: the lines of positions [p0, p1), ascending, as `name \t position + 1 \t cov \n': with all == 0 those with span > 0, otherwise every one.
 *   The text is written on the device and copied out once; *len: its bytes.  SSG_EOVERFLOW with *len set and nothing written when cap is too small; cap == 0
 *   with out == NULL is the sizing form and returns 0.
 * ssg_depth_end: closes the span and frees its memory.  Results do not depend on SSG_DEPTH_TILE (the positions of the accumulating kernel's LDS tile, 0 .. 8000,
 *   0: every add goes to global memory). */
typedef struct ssg_depth ssg_depth_t;
int  ssg_depth_create(ssg_recs_t *r, const ssg_bam_fop_t *prog, int n_prog, int min_baseq, ssg_depth_t **out);
int  ssg_depth_begin(ssg_depth_t *d, int32_t tid, int64_t beg, int64_t end);
int  ssg_depth_push(ssg_depth_t *d, uint32_t chunk_id, const uint64_t *hint, int64_t n_hints, uint64_t first, uint64_t *n_rec, uint64_t *n_used, uint64_t *n_later, uint64_t *descents, uint64_t *n_behind);
int  ssg_depth_finish(ssg_depth_t *d);
int  ssg_depth_get(ssg_depth_t *d, int64_t p0, int64_t p1, uint32_t *span_out, uint32_t *cov_out);
int  ssg_depth_sums(ssg_depth_t *d, const int64_t *reg, int64_t n_reg, const uint32_t *thr, int n_thr, uint64_t *out);
int  ssg_depth_text(ssg_depth_t *d, const char *name, int64_t p0, int64_t p1, int all, uint8_t *out, uint64_t cap, uint64_t *len);
int  ssg_depth_end(ssg_depth_t *d);
void ssg_depth_free(ssg_depth_t *d);

/* ---- the QC tables of `samtools stats' on the device (csrc/ssg_stats.cpp, k_stats.h; samtools 1.3.1 stats.c: the numbers are collect_stats' for a file read
 * whole, without -r, -t, -S, -I, -l, -q; the GC-depth table is not computed) ----
 * The stream is fed chunk by chunk (ssg_recs_append_bgzf, then ssg_stats_push).  Everything but the coverage histogram is a sum of per-record integers: any order
 * of the adds gives the same bits.  What a record adds, in collect_stats' order:
 *   - the filter program (the programs and fields of ssg_recs_select; what -f / -F / -d are to samtools) leaves 0: SSG_ST_FILTERED + 1, nothing else;
 *   - update_checksum: three CRC-32s (zlib's, initial value 0) are added into three 32-bit sums that wrap: the name up to its NUL, the (l_seq + 1) / 2 packed
 *     sequence bytes, and the FIRST (l_seq + 1) / 2 quality bytes (samtools' own count, kept); the last two only when l_seq > 0;
 *   - flag 0x100: SSG_ST_SECONDARY + 1 and nothing more; l_seq == 0: nothing more; flag 0x400: SSG_ST_DUP + 1, SSG_ST_DUP_LEN + l_seq;
 *   - unclipped_length: l_seq + the lengths of the H operations; SSG_ST_MAX_LEN is its maximum;
 *   - collect_orig_read_stats, for records with neither 0x100 nor 0x800: rl[unclipped length], total length, QC-fail, paired, first (0x80 clear) or last (0x80
 *     set) fragment; per base i the cycle is i, or l_seq - 1 - i with 0x10: bases[cycle][A, C, G, T, N, other] from the 4-bit codes 1, 2, 4, 8, 15 and the rest;
 *     quals[fragment][cycle][q] from the quality byte at l_seq - 1 - cycle with 0x10, else at cycle, with its sum and maximum; with g the C and G bases, the bins
 *     g * 199 / l_seq up to but excluding min((g + 1) * 199 / l_seq, 199) of gc[fragment] get + 1; then unmapped, or bases mapped, MQ0, single / paired-and-mapped,
 *     proper, mates on another contig, as the function has them;
 *   - flag 0x4 clear: count_indels -- operations of length 0 are skipped, an I at query offset c of a record of fragment f (0x40 set: 0, else 1) adds to
 *     ic[f][c] (ic[f][l_seq - c - len] with 0x10), a D to ic[2 + f][c - 1] (ic[2 + f][l_seq - c - 1] with 0x10; dropped when that is below 0), both to id[0 / 1][len - 1]
 *     up to length 300; N, H and P do not advance c;  the insert size: |isize| in 64 bits clamped to n_isize - 1, counted when it is > 0 or tid == mtid for
 *     records that are paired with both mates mapped, by collect_stats' orientation rule into isize[inward, outward, other]; the first NM tag of the aux area
 *     (walked with the types A c C s S i I f Z H B; any other type, a Z / H without NUL or a B cut short ends the walk) as bam_aux2i reads it (c C s S i I,
 *     anything else 0), added in 64-bit two's complement; the M and I lengths;
 *   - round_buffer_*: every such mapped record covers [pos, pos + l_seq - 1] (the read length, not the CIGAR; past a contig's end as well); cov[] is the
 *     histogram of the non-zero depths through coverage_idx(cov_min, cov_max, cov_step), n_cov = 3 + (cov_max - cov_min) / cov_step bins after samtools' own
 *     rounding of the three (ssg_stats_ncov).  This is the one order-dependent part: the records that get this far must not descend in (tid, pos), within a push
 *     or from one push to the next; from the first descent on SSG_ST_SORTED reads 0, cov[] is all 0 and stays so.  (samtools lets a contig recur; here that is a
 *     descent.)  The depths are kept as differences over a window of `span' positions plus max_len of slack that the object slides itself.
 * ssg_stats_create: opt->max_len: the longest unclipped length taken (1 .. 65535; the tables have max_len + 1 rows); n_isize 1 .. 2^24; 0 <= cov_min <= cov_max
 *   <= 2^24, cov_step >= 1, at most 8192 bins; span 1 .. 2^28, 0: 2^22.  SSG_EINVAL for these and for what ssg_recs_select refuses of a program.  The object
 *   lives on the store's device and must be freed before the store.
 * ssg_stats_push: the chunk's records are found as ssg_recs_scan finds them (the same hints, `first', SSG_EIO / SSG_EALIGN / SSG_EINVAL and words, under this
 *   entry's name).  *n_rec: the records scanned; *descents: the descents this push saw.  SSG_EIO for a record with 32 + l_qname + 4 n_cigar + (l_seq + 1) / 2 +
 *   l_seq > block_size, for a record that gets as far as count_indels with n_cigar == 0 (samtools aborts on it), and for an insertion or deletion whose cycle lies
 *   outside 0 .. max_len; SSG_ERANGE for an unclipped length above max_len (the record's offset in ssg_last_error()); SSG_EINVAL after ssg_stats_finish and while
 *   an order is declared.  On every failure the object's numbers are those from before the call.  The chunk is not released.
 * ssg_stats_finish: the window's last depths go into cov[]; no push after it.
 * ssg_stats_get: scalars[SSG_ST_N]; quals[2][max_len + 1][256]; bases[max_len + 1][6]; gc[2][200]; isize[3][n_isize], each pair having been counted twice and
 *   halved here with truncation, as output_stats does; rl[max_len + 1]; id[2][300]; ic[4][max_len + 1]; cov[n_cov]: 64-bit integers, a NULL pointer skips its
 *   table.  Allowed at any time; cov[] is complete after ssg_stats_finish.
 * Results do not depend on SSG_STATS_TILE (the cycles of the per-base kernel's LDS tile, 1 .. 32) or SSG_STATS_SLAB (the records a workgroup of it takes). */
enum { SSG_ST_FILTERED, SSG_ST_SECONDARY, SSG_ST_DUP, SSG_ST_DUP_LEN, SSG_ST_MAX_LEN, SSG_ST_TOTAL_LEN, SSG_ST_QCFAIL, SSG_ST_PAIRED, SSG_ST_FIRST, SSG_ST_LAST,
       SSG_ST_UNMAPPED, SSG_ST_BASES_MAPPED, SSG_ST_MQ0, SSG_ST_SINGLE, SSG_ST_PAIRED_MAPPED, SSG_ST_PROPER, SSG_ST_ANOMALOUS, SSG_ST_MISMATCHES, SSG_ST_BASES_CIGAR,
       SSG_ST_SUM_QUAL, SSG_ST_MAX_QUAL, SSG_ST_CHK_NAMES, SSG_ST_CHK_READS, SSG_ST_CHK_QUALS, SSG_ST_SORTED, SSG_ST_N = 32 };
#define SSG_STATS_NGC 200
#define SSG_STATS_NINDEL 300
typedef struct { int32_t max_len, n_isize, cov_min, cov_max, cov_step, span; } ssg_stats_opt_t;
typedef struct ssg_stats ssg_stats_t;
int64_t ssg_stats_ncov(const ssg_stats_opt_t *opt);   /* the bins of cov[] for these options; -1 for options ssg_stats_create refuses */
int  ssg_stats_create(ssg_recs_t *r, const ssg_bam_fop_t *prog, int n_prog, const ssg_stats_opt_t *opt, ssg_stats_t **out);
int  ssg_stats_push(ssg_stats_t *s, uint32_t chunk_id, const uint64_t *hint, int64_t n_hints, uint64_t first, uint64_t *n_rec, uint64_t *descents);
int  ssg_stats_finish(ssg_stats_t *s);
int  ssg_stats_get(ssg_stats_t *s, uint64_t *scalars, uint64_t *quals, uint64_t *bases, uint64_t *gc, uint64_t *isize, uint64_t *rl, uint64_t *id, uint64_t *ic, uint64_t *cov);
void ssg_stats_free(ssg_stats_t *s);

/* ---- `sambamba markdup' on the device (csrc/ssg_markdup.cpp, k_markdup.h): Picard MarkDuplicates' rule, as `sambamba markdup' documents it, over a stream that passes twice ----
 * The stream is the records of the pushes, in order (ssg_recs_append_bgzf, then ssg_markdup_push); a record's ordinal is its running number from 0.  Nothing
 * requires a coordinate-sorted stream: the decision is a global sort, not a sweep.
 *   Library: lib_of_rg[] of the record's RG:Z value -- the aux area walked as ssg_b2f_push walks it, the last RG:Z met -- and 0 without one or with a value that
 *     is not in rg[].  The caller maps @RG ID -> LB: equal LB strings share an id >= 1, an @RG without LB has 0.
 *   Taking part: flag & 0x904 clear and n_cigar > 0.  Every other record leaves as it came, its 0x400 included.
 *   End key of a taking-part record: (library, tid, u5, rev), rev = flag >> 4 & 1; u5 = pos - the lengths of the leading run of S and H operations (rev == 0),
 *     or end - 1 + the lengths of the trailing run of S and H operations (rev == 1, `end' as in ssg_bam_ent_t), in 64 bits.
 *   Score: the sum of the l_seq quality bytes that are >= 15, bytes taken unsigned, saturating at 2^30 - 1; 0 for l_seq == 0.
 *   Paired: a taking-part record with flag & 1 set and flag & 8 clear, by its flags alone.  The others are fragments.
 *   Mates: among the paired records of one name (l_qname - 1 bytes compared whole, library apart), in ordinal order: nothing held -- the record is held; the
 *     held one has the same flag & 0xc0 -- the record stays unmatched, the held one held; otherwise the two are a pair and nothing is held.
 *   Pair key: the two end keys ordered by (tid, u5, rev), the forward end first on a tie (Picard's RF -> FR), a lower library first when these are equal; pair
 *     score: the sum of the two scores; pair ordinal: the smaller of the two.
 *   Pairs: among pairs of one pair key the highest score is kept, on equal scores the smallest pair ordinal; both records of every other pair are duplicates.
 *   Fragments: among all taking-part records of one end key, if one of them is paired (matched or not) every fragment is a duplicate; otherwise the fragment
 *     with the highest score is kept, the smallest ordinal among equals, and the other fragments are duplicates.  A paired record is never marked by this step.
 *   Result: a taking-part record has 0x400 cleared, then set when it is a duplicate: one byte of the record.  With `remove' the duplicates leave instead.
 * ssg_markdup_create: rg[0 .. n_rg) are the @RG ids, lib_of_rg[] their libraries; hash_bits in 0 .. 64 is how much of the 64-bit name hash groups the paired
 *   records for the mate join -- results do not depend on it, callers pass 64.  The object lives on the store's device and must be freed before the store; its
 *   entries (40 bytes a record), the names of the paired records and the bitmap are device memory that counts against the store's capacity.  SSG_EINVAL for a
 *   NULL store, a NULL or empty id, n_rg < 0, no lib_of_rg[], hash_bits outside 0 .. 64.
 * ssg_markdup_push: the chunk's records are found as ssg_recs_scan finds them (the same hints, `first', SSG_EIO / SSG_EALIGN / SSG_EINVAL and words, under this
 *   entry's name).  SSG_EIO also for a record with 32 + l_qname + 4 n_cigar + (l_seq + 1) / 2 + l_seq > block_size (its offset in ssg_last_error());
 *   SSG_ENOMEM when the entries and names do not fit the store's capacity or the device; SSG_EINVAL after ssg_markdup_finish, while an order is declared, and
 *   past 2^32 - 16 records.  On every failure the object, the store and the chunk are as before and the call may be repeated.  On success the chunk is released.
 * ssg_markdup_finish: decides; counts[SSG_MD_N].  SSG_ERANGE when more than SSG_MARKDUP_RUN_MAX paired records share one name hash of hash_bits bits: the
 *   object is as before the call.  Zero records succeed.  After it only get, apply and free.
 * ssg_markdup_get: dup[k] = 1 when ordinal ord0 + k is a duplicate, else 0 (tests).  SSG_EINVAL before finish and past the records.
 * ssg_markdup_apply: the second pass -- the same stream's chunks, in the same order; the object keeps the running ordinal.  THIS ENTRY CHANGES RECORD BYTES: the
 *   flag byte that holds 0x400, in the store's chunk, of every taking-part record.  loc / ent of the kept records (all of them with remove == 0; ent.flag as
 *   patched) come back in stream order for ssg_recs_order; the chunk is not released.
 *     SSG_EINVAL     before finish; a chunk that runs past the records counted by the pushes; while an order is declared;
 *     SSG_EIO        a record whose block_size or name hash is not what its ordinal had in the first pass (the stream changed between the passes; the ordinal
 *                    in ssg_last_error());
 *     SSG_EOVERFLOW  cap < *n_kept: *n_rec and *n_kept are set, nothing is written.  cap == 0 with loc and ent NULL is the counting form: the two numbers.
 *   Nothing is patched and the running ordinal stays unless 0 is returned with the arrays written. */
#define SSG_MARKDUP_RUN_MAX 256
enum { SSG_MD_RECORDS, SSG_MD_TAKING_PART, SSG_MD_PAIRED, SSG_MD_PAIRS, SSG_MD_UNMATCHED, SSG_MD_FRAGMENTS, SSG_MD_DUP_PAIRED, SSG_MD_DUP_FRAGMENTS, SSG_MD_N = 16 };
typedef struct ssg_markdup ssg_markdup_t;
int  ssg_markdup_create(ssg_recs_t *r, const char *const *rg, const uint16_t *lib_of_rg, int n_rg, int hash_bits, ssg_markdup_t **out);
int  ssg_markdup_push(ssg_markdup_t *m, uint32_t chunk_id, const uint64_t *hint, int64_t n_hints, uint64_t first, uint64_t *n_rec);
int  ssg_markdup_finish(ssg_markdup_t *m, uint64_t *counts /* SSG_MD_N */);
int  ssg_markdup_get(ssg_markdup_t *m, uint64_t ord0, uint64_t n, uint8_t *dup);
int  ssg_markdup_apply(ssg_markdup_t *m, uint32_t chunk_id, const uint64_t *hint, int64_t n_hints, uint64_t first, int remove, uint64_t cap,
                       uint64_t *n_rec, uint64_t *n_kept, uint64_t *loc, ssg_bam_ent_t *ent);
void ssg_markdup_free(ssg_markdup_t *m);

#ifdef __cplusplus
}
#endif
#endif
