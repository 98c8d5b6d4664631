"""ctypes binding of libssgpu.so's C ABI (include/ssgpu.h).

The product library is the HIP build in this directory.  There is no CPU fallback: if the shared
object is missing or no GPU is visible the calls raise.  Tests may load the host-emulation build of
the same sources (tests/emu/libssgpu_emu.so) by passing its path explicitly.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "libssgpu.so")

# numpy mirrors of speedseq_amd/csrc/ssg_types.h
OPT_DT = np.dtype([
    ("a", "i4"), ("b", "i4"), ("o_del", "i4"), ("e_del", "i4"), ("o_ins", "i4"), ("e_ins", "i4"),
    ("pen_unpaired", "i4"), ("pen_clip5", "i4"), ("pen_clip3", "i4"), ("w", "i4"), ("zdrop", "i4"),
    ("T", "i4"), ("min_seed_len", "i4"), ("min_chain_weight", "i4"), ("max_chain_extend", "i4"),
    ("split_width", "i4"), ("max_occ", "i4"), ("max_chain_gap", "i4"), ("max_ins", "i4"), ("max_matesw", "i4"),
    ("max_XA_hits", "i4"), ("max_XA_hits_alt", "i4"), ("mapQ_coef_fac", "i4"), ("chunk_size", "i4"), ("n_threads", "i4"),
    ("_align", "i4"),
    ("max_mem_intv", "u8"),
    ("split_factor", "f4"), ("mask_level", "f4"), ("drop_ratio", "f4"), ("XA_drop_ratio", "f4"),
    ("mask_level_redun", "f4"), ("mapQ_coef_len", "f4"),
    ("mat", "i1", (25,)), ("_pad0", "i1"), ("flag", "u2"), ("_pad", "i1", (4,)),
], align=False)
INTV_DT = np.dtype([("x0", "u8"), ("x1", "u8"), ("x2", "u8"), ("info", "u8")])
SEED_DT = np.dtype([("rbeg", "i8"), ("qbeg", "i4"), ("len", "i4"), ("score", "i4"), ("next", "i4")])
CHAIN_DT = np.dtype([("pos", "i8"), ("first_seed", "i4"), ("last_seed", "i4"), ("n", "i4"), ("rid", "i4"), ("w", "i4"), ("kept", "i4"), ("first", "i4"), ("sec", "i4"),
                     ("left", "i4"), ("right", "i4"), ("frac_rep", "f4"), ("_pad", "i4")])
# ssg_dbg_chain's form[]: the kernel that chained a read (include/ssgpu.h SSG_CHAIN_FORM_*)
CHAIN_FORM_LANE, CHAIN_FORM_LDS16, CHAIN_FORM_LDS32, CHAIN_FORM_LDS64 = 0, 1, 2, 3
CHAIN_FORM_WAVE256, CHAIN_FORM_WAVE512, CHAIN_FORM_WAVE1024, CHAIN_FORM_WAVE2048, CHAIN_FORM_WAVE5120 = 4, 5, 6, 7, 8
CHAIN_FORM_TREE = 0x10
# ssg_dbg_regions' route[] bits (include/ssgpu.h SSG_REG_ROUTE_*)
REG_ROUTE_WAVE, REG_ROUTE_PATCH = 1, 2
# ssg_dbg_reg2aln's route[] bits (include/ssgpu.h SSG_R2A_ROUTE_*)
R2A_ROUTE_LANE, R2A_ROUTE_DP0, R2A_ROUTE_DP1, R2A_ROUTE_DP2, R2A_ROUTE_WAVE = 1, 2, 4, 8, 16
EXT_JOB_DT = np.dtype([("qoff", "i4"), ("qlen", "i4"), ("toff", "i4"), ("tlen", "i4"), ("w", "i4"), ("end_bonus", "i4"), ("zdrop", "i4"), ("h0", "i4")])
EXT_RES_DT = np.dtype([("score", "i4"), ("qle", "i4"), ("tle", "i4"), ("gtle", "i4"), ("gscore", "i4"), ("max_off", "i4")])
SW_JOB_DT = np.dtype([("qoff", "i4"), ("qlen", "i4"), ("toff", "i4"), ("tlen", "i4"), ("xtra", "i4"), ("_pad", "i4")])
KSWR_DT = np.dtype([("score", "i4"), ("te", "i4"), ("qe", "i4"), ("score2", "i4"), ("te2", "i4"), ("tb", "i4"), ("qb", "i4")])
GLB_JOB_DT = np.dtype([("qoff", "i4"), ("qlen", "i4"), ("toff", "i4"), ("tlen", "i4"), ("w", "i4"), ("_pad", "i4")])
ALNREG_DT = np.dtype([
    ("rb", "i8"), ("re", "i8"), ("qb", "i4"), ("qe", "i4"), ("rid", "i4"), ("score", "i4"), ("truesc", "i4"), ("sub", "i4"),
    ("alt_sc", "i4"), ("csub", "i4"), ("sub_n", "i4"), ("w", "i4"), ("seedcov", "i4"), ("secondary", "i4"),
    ("secondary_all", "i4"), ("seedlen0", "i4"), ("n_comp", "i4"), ("frac_rep", "f4"), ("hash", "u8"),
])
PESTAT_DT = np.dtype([("low", "i4"), ("high", "i4"), ("failed", "i4"), ("_pad", "i4"), ("avg", "f8"), ("std", "f8")])


class SsgError(RuntimeError):
    pass


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Lib:
    def __init__(self, path=None):
        path = path or os.environ.get("SSGPU_LIB") or DEFAULT_LIB   # SSGPU_LIB: e.g. the instrumented build of `make tune`
        if not os.path.exists(path):
            raise SsgError("%s not found: build it with `make lib` (hipcc --offload-arch=gfx950); there is no CPU fallback" % path)
        self.path = path
        self.l = C.CDLL(path)
        self.l.ssg_version.restype = C.c_char_p
        self.l.ssg_backend.restype = C.c_char_p
        self.l.ssg_last_error.restype = C.c_char_p
        self.l.ssg_index_l_pac.restype = C.c_int64
        assert OPT_DT.itemsize == self.sizeof_opt(), (OPT_DT.itemsize, self.sizeof_opt())

    def sizeof_opt(self):
        # ssg_mem_opt_t: 25 int32 (+4 pad) + u64 + 6 floats + 32 bytes
        return 25 * 4 + 4 + 8 + 6 * 4 + 32

    def _chk(self, rc):
        if rc != 0:
            raise SsgError("libssgpu error %d: %s" % (rc, self.l.ssg_last_error().decode()))

    def backend(self):
        return self.l.ssg_backend().decode()

    def device_count(self):
        return self.l.ssg_device_count()

    def opt_init(self):
        o = np.zeros(1, dtype=OPT_DT)
        self.l.ssg_mem_opt_init(_ptr(o))
        return o

    # ---- index ----
    def index_load(self, prefix):
        h = C.c_void_p()
        self._chk(self.l.ssg_index_load(prefix.encode(), C.byref(h)))
        return h

    def index_build_fasta(self, fasta):
        """upstream `bwa index` on the GPU (ssg_index_build_fasta); returns the index handle."""
        h = C.c_void_p()
        self._chk(self.l.ssg_index_build_fasta(fasta.encode(), C.byref(h)))
        return h

    def index_build_dev(self, d_fwd, l_pac, ctg_off, ctg_len, names=None):
        """index of forward-strand nt4 codes resident in HBM (d_fwd = device address)."""
        h = C.c_void_p()
        co = np.asarray(ctg_off, dtype=np.int64)
        cl = np.asarray(ctg_len, dtype=np.int32)
        self._chk(self.l.ssg_index_build_dev(C.c_void_p(d_fwd), C.c_int64(l_pac), C.c_int(len(co)), _ptr(co), _ptr(cl), C.byref(h)))
        if names is not None:
            arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
            self._chk(self.l.ssg_index_set_names(h, C.c_int(len(names)), arr))
        return h

    def index_save(self, h, prefix):
        self._chk(self.l.ssg_index_save(h, prefix.encode()))

    def index_destroy(self, h):
        self.l.ssg_index_destroy(h)

    # ---- stage-level ----
    def extend_batch(self, opt, jobs, qbuf, tbuf):
        jobs = np.ascontiguousarray(jobs, dtype=EXT_JOB_DT)
        res = np.zeros(len(jobs), dtype=EXT_RES_DT)
        cells = C.c_uint64(0)
        self._chk(self.l.ssg_extend_batch(_ptr(opt), C.c_int(len(jobs)), _ptr(jobs), _ptr(qbuf), C.c_size_t(qbuf.size),
                                          _ptr(tbuf), C.c_size_t(tbuf.size), _ptr(res), C.byref(cells)))
        return res, cells.value

    def align2_batch(self, opt, jobs, qbuf, tbuf):
        jobs = np.ascontiguousarray(jobs, dtype=SW_JOB_DT)
        res = np.zeros(len(jobs), dtype=KSWR_DT)
        self._chk(self.l.ssg_align2_batch(_ptr(opt), C.c_int(len(jobs)), _ptr(jobs), _ptr(qbuf), C.c_size_t(qbuf.size),
                                          _ptr(tbuf), C.c_size_t(tbuf.size), _ptr(res)))
        return res

    def global_batch(self, opt, jobs, qbuf, tbuf, cap=64):
        jobs = np.ascontiguousarray(jobs, dtype=GLB_JOB_DT)
        n = len(jobs)
        score = np.zeros(n, dtype=np.int32)
        ncig = np.zeros(n, dtype=np.int32)
        cig = np.zeros((n, cap), dtype=np.uint32)
        self._chk(self.l.ssg_global_batch(_ptr(opt), C.c_int(n), _ptr(jobs), _ptr(qbuf), C.c_size_t(qbuf.size),
                                          _ptr(tbuf), C.c_size_t(tbuf.size), _ptr(score), _ptr(ncig), _ptr(cig), C.c_int(cap)))
        return score, ncig, cig

    def smem_batch(self, idx, opt, seq, off, cap=64):
        n = len(off) - 1
        intv = np.zeros((n, cap), dtype=INTV_DT)
        cnt = np.zeros(n, dtype=np.int32)
        self._chk(self.l.ssg_smem_batch(idx, _ptr(opt), C.c_int(n), _ptr(seq), _ptr(off), C.c_int(cap), _ptr(intv), _ptr(cnt)))
        return intv, cnt

    def dbg_smem_ext(self, idx, opt, seq, off, cap=64):
        """the seeding stage's two kernels alone (ssg_dbg_smem_ext): (intervals unsorted, counts, upstream's bwt_extend count over the reads, the wave
        kernel's reads by how it took them up: resumed in pass 1 at x > 0, resumed in pass 2, started again for an unfinished third pass, pass 1 from the start)"""
        n = len(off) - 1
        intv = np.zeros((n, cap), dtype=INTV_DT)
        cnt = np.zeros(n, dtype=np.int32)
        nx = C.c_uint64(0)
        paths = np.zeros(4, dtype=np.uint32)
        self._chk(self.l.ssg_dbg_smem_ext(idx, _ptr(opt), C.c_int(n), _ptr(seq), _ptr(off), C.c_int(cap), _ptr(intv), _ptr(cnt), C.byref(nx), _ptr(paths)))
        return intv, cnt, nx.value, [int(x) for x in paths]

    def dbg_extend_coop(self, idx, intv, base, is_back):
        """one bwt_extend per item by ssg_bwt_extend1_lean and by s2_extend_coop, and four at a time by the former and by s2_extend_coop4 (ssg_dbg_extend_coop):
        (lean, coop [INTV_DT, n], lean4, coop4 [INTV_DT, n x 4]: item t's base and direction on the intervals of items t .. t + 3 mod n)"""
        intv = np.ascontiguousarray(intv, dtype=INTV_DT)
        base, is_back = np.ascontiguousarray(base, dtype=np.uint8), np.ascontiguousarray(is_back, dtype=np.uint8)
        n = len(intv)
        lean, coop, lean4, coop4 = np.zeros(n, dtype=INTV_DT), np.zeros(n, dtype=INTV_DT), np.zeros((n, 4), dtype=INTV_DT), np.zeros((n, 4), dtype=INTV_DT)
        self._chk(self.l.ssg_dbg_extend_coop(idx, C.c_int(n), _ptr(intv), _ptr(base), _ptr(is_back), _ptr(lean), _ptr(coop), _ptr(lean4), _ptr(coop4)))
        return lean, coop, lean4, coop4

    def seeds_batch(self, idx, opt, seq, off):
        """seeds of every read before chaining: (seed_off, seeds[rbeg qbeg len score next], rids)"""
        n = len(off) - 1
        seed_off = np.zeros(n + 1, dtype=np.int64)
        sp, rp = C.c_void_p(), C.c_void_p()
        self._chk(self.l.ssg_seeds_batch(idx, _ptr(opt), C.c_int(n), _ptr(seq), _ptr(off), _ptr(seed_off), C.byref(sp), C.byref(rp)))
        tot = int(seed_off[n])
        seeds = np.frombuffer((C.c_char * (tot * SEED_DT.itemsize)).from_address(sp.value), dtype=SEED_DT, count=tot).copy() if tot else np.zeros(0, SEED_DT)
        rids = np.frombuffer((C.c_char * (tot * 4)).from_address(rp.value), dtype=np.int32, count=tot).copy() if tot else np.zeros(0, np.int32)
        self.l.ssg_free(sp); self.l.ssg_free(rp)
        return seed_off, seeds, rids

    def extend_lane_batch(self, idx, opt, jobs, tpos, direction, qbuf, qcap):
        res = np.zeros(len(jobs), dtype=EXT_RES_DT)
        cells = C.c_uint64(0)
        tpos = np.ascontiguousarray(tpos, dtype=np.int64)
        self._chk(self.l.ssg_extend_lane_batch(idx, _ptr(opt), C.c_int(len(jobs)), _ptr(jobs), _ptr(tpos), C.c_int(direction), _ptr(qbuf), C.c_size_t(qbuf.size), C.c_int(qcap), _ptr(res), C.byref(cells)))
        return res, cells.value

    def align2_lane_batch(self, idx, opt, jobs, tpos, qbuf, lanes):
        jobs = np.ascontiguousarray(jobs, dtype=SW_JOB_DT)
        res = np.zeros(len(jobs), dtype=KSWR_DT)
        from_lane = np.zeros(len(jobs), dtype=np.int32)
        tpos = np.ascontiguousarray(tpos, dtype=np.int64)
        self._chk(self.l.ssg_align2_lane_batch(idx, _ptr(opt), C.c_int(len(jobs)), _ptr(jobs), _ptr(tpos), _ptr(qbuf), C.c_size_t(qbuf.size), C.c_int(lanes), _ptr(res), _ptr(from_lane)))
        return res, from_lane

    def dbg_chain_sort(self, keys):
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        o0, o1 = np.zeros(len(keys), dtype=np.int64), np.zeros(len(keys), dtype=np.int64)
        self._chk(self.l.ssg_dbg_chain_sort(_ptr(keys), C.c_int(len(keys)), _ptr(o0), _ptr(o1)))
        return o0, o1

    def dbg_chain(self, opt, l_pac, n_ctg, read_len, seed_off, seeds, rids, intv_off, intv):
        """the chaining stage on given seeds and intervals (ssg_dbg_chain): (chain_off, surviving chains in final order [CHAIN_DT; first_seed = offset into the
        next array], their seed indices counted from the read's first seed, the kernel form that took each read [CHAIN_FORM_*])"""
        read_len = np.ascontiguousarray(read_len, dtype=np.int32)
        seed_off = np.ascontiguousarray(seed_off, dtype=np.int64)
        intv_off = np.ascontiguousarray(intv_off, dtype=np.int64)
        seeds = np.ascontiguousarray(seeds, dtype=SEED_DT)
        rids = np.ascontiguousarray(rids, dtype=np.int32)
        intv = np.ascontiguousarray(intv, dtype=INTV_DT)
        n = len(read_len)
        assert len(seed_off) == n + 1 and len(intv_off) == n + 1 and len(seeds) >= seed_off[-1] and len(rids) >= seed_off[-1] and len(intv) >= intv_off[-1]
        chain_off, form = np.zeros(n + 1, dtype=np.int64), np.zeros(n, dtype=np.int32)
        cp, sp = C.c_void_p(), C.c_void_p()
        self._chk(self.l.ssg_dbg_chain(_ptr(opt), C.c_int64(l_pac), C.c_int(n_ctg), C.c_int(n), _ptr(read_len), _ptr(seed_off), _ptr(seeds), _ptr(rids), _ptr(intv_off), _ptr(intv),
                                       _ptr(chain_off), C.byref(cp), C.byref(sp), _ptr(form)))
        nc = int(chain_off[n])
        chains = np.frombuffer((C.c_char * (nc * CHAIN_DT.itemsize)).from_address(cp.value), dtype=CHAIN_DT, count=nc).copy() if nc else np.zeros(0, CHAIN_DT)
        ns = int(chains["n"].sum()) if nc else 0
        cseeds = np.frombuffer((C.c_char * (ns * 4)).from_address(sp.value), dtype=np.int32, count=ns).copy() if ns else np.zeros(0, np.int32)
        self.l.ssg_free(cp); self.l.ssg_free(sp)
        return chain_off, chains, cseeds, form

    def dbg_regions(self, opt, pac, l_pac, ctg_off, ctg_len, seq, off, seed_off, seeds, chain_off, chains, chain_seeds):
        """the region stage on given chains (ssg_dbg_regions; chains and chain_seeds in the form dbg_chain returns): (reg_off, regions [ALNREG_DT], route per read
        [REG_ROUTE_* bits])"""
        pac = np.ascontiguousarray(pac, dtype=np.uint8)
        ctg_off = np.ascontiguousarray(ctg_off, dtype=np.int64)
        ctg_len = np.ascontiguousarray(ctg_len, dtype=np.int32)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        seed_off = np.ascontiguousarray(seed_off, dtype=np.int64)
        chain_off = np.ascontiguousarray(chain_off, dtype=np.int64)
        seeds = np.ascontiguousarray(seeds, dtype=SEED_DT)
        chains = np.ascontiguousarray(chains, dtype=CHAIN_DT)
        chain_seeds = np.ascontiguousarray(chain_seeds, dtype=np.int32)
        n = len(off) - 1
        assert len(pac) >= l_pac // 4 + 1 and len(ctg_off) == len(ctg_len) and len(seed_off) == n + 1 and len(chain_off) == n + 1
        assert len(seq) >= off[-1] and len(seeds) >= seed_off[-1] and len(chains) >= chain_off[-1] and len(chain_seeds) >= int(chains["n"][:int(chain_off[-1])].sum())
        reg_off, route = np.zeros(n + 1, dtype=np.int64), np.zeros(n, dtype=np.int32)
        rp = C.c_void_p()
        self._chk(self.l.ssg_dbg_regions(_ptr(opt), _ptr(pac), C.c_int64(l_pac), C.c_int(len(ctg_off)), _ptr(ctg_off), _ptr(ctg_len), C.c_int(n), _ptr(seq), _ptr(off),
                                         _ptr(seed_off), _ptr(seeds), _ptr(chain_off), _ptr(chains), _ptr(chain_seeds), _ptr(reg_off), C.byref(rp), _ptr(route)))
        tot = int(reg_off[n])
        regs = np.frombuffer((C.c_char * (tot * ALNREG_DT.itemsize)).from_address(rp.value), dtype=ALNREG_DT, count=tot).copy() if tot else np.zeros(0, ALNREG_DT)
        self.l.ssg_free(rp)
        return reg_off, regs, route

    def dbg_reg2aln(self, opt, pac, l_pac, ctg_off, ctg_len, seq, off, regs, req):
        """the record stage on given regions and requests (ssg_dbg_reg2aln): (return code, records [ALN_DT], route per request [R2A_ROUTE_* bits], the stage's device
        error code).  The return code is 0 or SSG_EOVERFLOW (-75: the device error code is not 0); every other code raises."""
        pac = np.ascontiguousarray(pac, dtype=np.uint8)
        ctg_off = np.ascontiguousarray(ctg_off, dtype=np.int64)
        ctg_len = np.ascontiguousarray(ctg_len, dtype=np.int32)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        regs = np.ascontiguousarray(regs, dtype=ALNREG_DT)
        req = np.ascontiguousarray(req, dtype=ALNREQ_DT)
        n = len(off) - 1
        assert len(pac) >= l_pac // 4 + 1 and len(ctg_off) == len(ctg_len) and n >= 0 and (n == 0 or len(seq) >= off[-1])
        alns, route, err = np.zeros(len(req) + 1, dtype=ALN_DT), np.zeros(len(req) + 1, dtype=np.int32), C.c_int32(0)
        rc = self.l.ssg_dbg_reg2aln(_ptr(opt), _ptr(pac), C.c_int64(l_pac), C.c_int(len(ctg_off)), _ptr(ctg_off), _ptr(ctg_len), C.c_int(n), _ptr(seq), _ptr(off),
                                    C.c_int64(len(regs)), _ptr(regs), C.c_int64(len(req)), _ptr(req), _ptr(alns), _ptr(route), C.byref(err))
        if rc != -75:
            self._chk(rc)
        return rc, alns[:len(req)], route[:len(req)], int(err.value)

    def dbg_pestat(self, idx, opt, reg_off, regs, pair_batch, n_batches):
        """mem_pestat on given region lists (ssg_dbg_pestat): n_batches x 4 insert-size models"""
        reg_off = np.ascontiguousarray(reg_off, dtype=np.int64)
        regs = np.ascontiguousarray(regs, dtype=ALNREG_DT)
        pair_batch = np.ascontiguousarray(pair_batch, dtype=np.int32)
        pes = np.zeros(4 * n_batches, dtype=PESTAT_DT)
        self._chk(self.l.ssg_dbg_pestat(idx, _ptr(opt), C.c_int((len(reg_off) - 1) // 2), _ptr(reg_off), _ptr(regs), _ptr(pair_batch), C.c_int(n_batches), _ptr(pes)))
        return pes

    def dbg_pair_final(self, idx, opt, id0, reg_off, regs, pes):
        """primary marking, pairing, MAPQ and record selection on given region lists (ssg_dbg_pair_final): (regions as the stage leaves them, req_off, requests)"""
        reg_off = np.ascontiguousarray(reg_off, dtype=np.int64)
        regs = np.ascontiguousarray(regs, dtype=ALNREG_DT)
        pes = np.ascontiguousarray(pes, dtype=PESTAT_DT)
        assert len(pes) == 4 and len(regs) == reg_off[-1]
        n = len(reg_off) - 1
        out = np.zeros(len(regs), dtype=ALNREG_DT)
        req_off = np.zeros(n + 1, dtype=np.int64)
        req_p = C.c_void_p()
        self._chk(self.l.ssg_dbg_pair_final(idx, _ptr(opt), C.c_int(n // 2), C.c_int64(id0), _ptr(reg_off), _ptr(regs), _ptr(pes), _ptr(out), _ptr(req_off), C.byref(req_p)))
        nreq = int(req_off[n])
        req = np.frombuffer((C.c_char * (nreq * ALNREQ_DT.itemsize)).from_address(req_p.value), dtype=ALNREQ_DT, count=nreq).copy() if nreq else np.zeros(0, ALNREQ_DT)
        self.l.ssg_free(req_p)
        return out, req_off, req

    def dbg_matesw(self, idx, opt, seq, read_off, reg_off, regs, pes, fixed=None, headroom=-1):
        """mate rescue on given region lists (ssg_dbg_matesw): (per-read lists after rescue, per-pair error codes, counts: windows, windows from slots,
        pairs decided on keys, pairs left to the record kernel, listed pairs, SW cells)"""
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        reg_off = np.ascontiguousarray(reg_off, dtype=np.int64)
        regs = np.ascontiguousarray(regs, dtype=ALNREG_DT)
        pes = np.ascontiguousarray(pes, dtype=PESTAT_DT)
        n = len(reg_off) - 1
        assert len(pes) == 4 and len(regs) == reg_off[-1] and len(read_off) == n + 1 and len(seq) == read_off[-1]
        fx = None if fixed is None else np.ascontiguousarray(fixed, dtype=np.uint8)
        assert fx is None or len(fx) == n
        out_off, n_out, err, counts = np.zeros(n + 1, dtype=np.int64), np.zeros(n, dtype=np.int32), np.zeros(n // 2, dtype=np.int32), np.zeros(8, dtype=np.uint64)
        out_p = C.c_void_p()
        self._chk(self.l.ssg_dbg_matesw(idx, _ptr(opt), C.c_int(n // 2), _ptr(seq), _ptr(read_off), _ptr(reg_off), _ptr(regs), _ptr(fx) if fx is not None else None, _ptr(pes),
                                        C.c_int(headroom), _ptr(out_off), C.byref(out_p), _ptr(n_out), _ptr(err), _ptr(counts)))
        tot = int(out_off[n])
        allr = np.frombuffer((C.c_char * (tot * ALNREG_DT.itemsize)).from_address(out_p.value), dtype=ALNREG_DT, count=tot).copy() if tot and out_p.value else np.zeros(0, ALNREG_DT)
        self.l.ssg_free(out_p)
        lists = [allr[int(out_off[r]):int(out_off[r]) + int(n_out[r])].copy() for r in range(n)]
        return lists, err, counts

    def dbg_matesw_last(self):
        """the counts of ssg_dbg_matesw for the calling thread's last rescue stage (the pipeline's included)"""
        counts = np.zeros(8, dtype=np.uint64)
        self.l.ssg_dbg_matesw_last(_ptr(counts))
        return counts

    def align1_batch(self, idx, opt, seq, off):
        n = len(off) - 1
        reg_off = np.zeros(n + 1, dtype=np.int64)
        regs_p = C.c_void_p()
        stats = np.zeros(8, dtype=np.uint64)
        self._chk(self.l.ssg_align1_batch(idx, _ptr(opt), C.c_int(n), _ptr(seq), _ptr(off), _ptr(reg_off), C.byref(regs_p), _ptr(stats)))
        tot = int(reg_off[n])
        buf = (C.c_char * (tot * ALNREG_DT.itemsize)).from_address(regs_p.value) if tot else b""
        regs = np.frombuffer(buf, dtype=ALNREG_DT, count=tot).copy()
        self.l.ssg_free(regs_p)
        return reg_off, regs, stats


ALNREQ_DT = np.dtype([("read", "i4"), ("reg", "i4"), ("kind", "i4"), ("owner", "i4"), ("flag", "i4"), ("mapq", "i4"), ("_p0", "i4"), ("_p1", "i4")])
ALN_DT = np.dtype([("pos", "i8"), ("rid", "i4"), ("flag", "i4"), ("mapq", "i4"), ("NM", "i4"), ("score", "i4"), ("sub", "i4"), ("n_cigar", "i4"),
                   ("is_rev", "i4"), ("l_md", "i4"), ("reg_idx", "i4"), ("xa_cnt", "i4"), ("_pad", "i4"), ("cigar", "u4", (64,)), ("md", "S320")])


class PeResult:
    """Owner of an ssg_pe_result_t (records of one ssg_mem_process_pairs call)."""

    def __init__(self, lib, handle, n_pairs, n_batches):
        self.lib, self.h, self.n_pairs, self.n_batches = lib, handle, n_pairs, n_batches
        l = lib.l
        n = l.ssg_pe_n_req(handle)
        self.req_off = np.ctypeslib.as_array(C.cast(l.ssg_pe_req_off(handle), C.POINTER(C.c_int64)), shape=(2 * n_pairs + 1,)).copy()
        self.req = np.frombuffer((C.c_char * (n * ALNREQ_DT.itemsize)).from_address(l.ssg_pe_req(handle)), dtype=ALNREQ_DT, count=n).copy() if n else np.zeros(0, ALNREQ_DT)
        self.alns = np.frombuffer((C.c_char * (n * ALN_DT.itemsize)).from_address(l.ssg_pe_alns(handle)), dtype=ALN_DT, count=n).copy() if n else np.zeros(0, ALN_DT)
        self.pes = np.frombuffer((C.c_char * (n_batches * 4 * PESTAT_DT.itemsize)).from_address(l.ssg_pe_pes(handle)), dtype=PESTAT_DT, count=n_batches * 4).copy() if n_batches else np.zeros(0, PESTAT_DT)
        self.stats = np.ctypeslib.as_array(C.cast(l.ssg_pe_stats(handle), C.POINTER(C.c_uint64)), shape=(8,)).copy()

    def close(self):
        if self.h:
            self.lib.l.ssg_pe_result_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


def _bind_pe(lib):
    l = lib.l
    l.ssg_pe_n_req.restype = C.c_int64
    for f in ("ssg_pe_req_off", "ssg_pe_req", "ssg_pe_alns", "ssg_pe_pes", "ssg_pe_stats"):
        getattr(l, f).restype = C.c_void_p
        getattr(l, f).argtypes = [C.c_void_p]
    l.ssg_pe_n_req.argtypes = [C.c_void_p]
    l.ssg_pe_result_free.argtypes = [C.c_void_p]


def mem_process_pairs(lib, idx, opt, seq, off, pair_batch=None, n_batches=1, id0=0, pes0=None):
    _bind_pe(lib)
    n_pairs = (len(off) - 1) // 2
    if pair_batch is None:
        pair_batch = np.zeros(n_pairs, dtype=np.int32)
    pair_batch = np.ascontiguousarray(pair_batch, dtype=np.int32)
    h = C.c_void_p()
    p0 = _ptr(pes0) if pes0 is not None else None
    lib._chk(lib.l.ssg_mem_process_pairs(idx, _ptr(opt), C.c_int(n_pairs), _ptr(seq), _ptr(off), _ptr(pair_batch), C.c_int(n_batches),
                                         C.c_int64(id0), p0, C.byref(h)))
    return PeResult(lib, h, n_pairs, n_batches)


SBL_END_DT = np.dtype([("seq", "i4"), ("pos", "i4"), ("flag", "i4"), ("lclip", "i4"), ("rclip", "i4"), ("ralen", "i4")])


def sbl_markdup(lib, ends):
    """ends: SBL_END_DT array of 2*n_pairs primary records -> uint8 dup flag per pair."""
    ends = np.ascontiguousarray(ends, dtype=SBL_END_DT)
    n = len(ends) // 2
    dup = np.zeros(n, dtype=np.uint8)
    lib._chk(lib.l.ssg_sbl_markdup(C.c_long(n), _ptr(ends), _ptr(dup)))
    return dup


SBL_LINE_DT = np.dtype([("seq", "i4"), ("pos", "i4"), ("flag", "i4"), ("mapq", "i4"), ("lclip", "i4"), ("rclip", "i4"), ("qalen", "i4"), ("ralen", "i4")])
SBL_OPT_DT = np.dtype([("exclude_dups", "i4"), ("add_mate_tags", "i4"), ("max_split_count", "i4"), ("min_non_overlap", "i4"), ("max_unmapped_bases", "i4"),
                       ("min_indel_size", "i4")])


def sbl_opt_init(lib, **kw):
    """ssg_sbl_opt_t with upstream samblaster's defaults, then the fields given"""
    o = np.zeros((), dtype=SBL_OPT_DT)
    lib.l.ssg_sbl_opt_init(_ptr(o))
    for k, v in kw.items():
        o[k] = v
    return o


def sbl_state_new(lib):
    lib.l.ssg_sbl_state_new.restype = C.c_void_p
    return C.c_void_p(lib.l.ssg_sbl_state_new())


def sbl_state_free(lib, st):
    lib.l.ssg_sbl_state_free(st)


def sbl_markdup_stream(lib, st, ends):
    """ssg_sbl_markdup_stream: like sbl_markdup, against the duplicate set that st keeps between calls"""
    ends = np.ascontiguousarray(ends, dtype=SBL_END_DT)
    n = len(ends) // 2
    dup = np.zeros(n, dtype=np.uint8)
    lib._chk(lib.l.ssg_sbl_markdup_stream(st, C.c_long(n), _ptr(ends), _ptr(dup)))
    return dup


def _sbl_chunk(blk_off, lines):
    off = np.ascontiguousarray(blk_off, dtype=np.int64)
    lines = np.ascontiguousarray(lines, dtype=SBL_LINE_DT)
    assert int(off[-1]) == len(lines), (int(off[-1]), len(lines))
    return off, lines, len(off) - 1


def sbl_process(lib, st, opt, blk_off, lines):
    """ssg_sbl_process over a chunk of name-grouped blocks (st may be None): (SSG_SBL_* bits, mate line) per line"""
    off, lines, nb = _sbl_chunk(blk_off, lines)
    bits, mate = np.zeros(len(lines), dtype=np.uint8), np.zeros(len(lines), dtype=np.int64)
    lib._chk(lib.l.ssg_sbl_process(st, _ptr(opt), C.c_long(nb), _ptr(off), _ptr(lines), _ptr(bits), _ptr(mate)))
    return bits, mate


def sbl_ends(lib, blk_off, lines):
    """ssg_sbl_ends: the two primary ends of every block (SBL_END_DT, 2 per block)"""
    off, lines, nb = _sbl_chunk(blk_off, lines)
    ends = np.zeros(2 * nb, dtype=SBL_END_DT)
    lib._chk(lib.l.ssg_sbl_ends(C.c_long(nb), _ptr(off), _ptr(lines), _ptr(ends)))
    return ends


def sbl_classify(lib, opt, blk_off, lines, dup):
    """ssg_sbl_classify: the lines classified with duplicate verdicts decided elsewhere (one byte per block)"""
    off, lines, nb = _sbl_chunk(blk_off, lines)
    dup = np.ascontiguousarray(dup, dtype=np.uint8)
    assert len(dup) == nb
    bits, mate = np.zeros(len(lines), dtype=np.uint8), np.zeros(len(lines), dtype=np.int64)
    lib._chk(lib.l.ssg_sbl_classify(_ptr(opt), C.c_long(nb), _ptr(off), _ptr(lines), _ptr(dup), _ptr(bits), _ptr(mate)))
    return bits, mate


def dbg_sbl_records(lib, req_off, req, alns, opt, st=None):
    """ssg_dbg_sbl_records: samblaster's stage of the timed step on given records.  (return code, dict of line_off, lines [SBL_LINE_DT], line_req, ends
    [SBL_END_DT], prim, sig [n_pairs x 3], dup, bits, mate, counts [4], keys); a refusal comes back as its code, the message in ssg_last_error."""
    req_off = np.ascontiguousarray(req_off, dtype=np.int64)
    req = np.ascontiguousarray(req, dtype=ALNREQ_DT)
    alns = np.ascontiguousarray(alns, dtype=ALN_DT)
    n_pairs, cap = (len(req_off) - 1) // 2, len(req) + 1
    assert len(req_off) == 2 * n_pairs + 1 and len(req) == len(alns)
    o = dict(line_off=np.zeros(n_pairs + 1, np.int64), lines=np.zeros(cap, SBL_LINE_DT), line_req=np.zeros(cap, np.int64), ends=np.zeros(2 * n_pairs + 1, SBL_END_DT),
             prim=np.zeros(2 * n_pairs + 1, np.int64), sig=np.zeros((n_pairs + 1, 3), np.uint64), dup=np.zeros(n_pairs + 1, np.uint8), bits=np.zeros(cap, np.uint8),
             mate=np.zeros(cap, np.int64), counts=np.zeros(4, np.uint64), keys=np.zeros(cap, np.uint64))
    nl = C.c_int64(0)
    rc = lib.l.ssg_dbg_sbl_records(C.c_long(n_pairs), _ptr(req_off), _ptr(req), _ptr(alns), _ptr(opt), st, _ptr(o["line_off"]), C.byref(nl), _ptr(o["lines"]),
                                   _ptr(o["line_req"]), _ptr(o["ends"]), _ptr(o["prim"]), _ptr(o["sig"]), _ptr(o["dup"]), _ptr(o["bits"]), _ptr(o["mate"]),
                                   _ptr(o["counts"]), _ptr(o["keys"]))
    n = int(nl.value)
    for k in ("lines", "line_req", "bits", "mate", "keys"):
        o[k] = o[k][:n]
    for k, m in (("ends", 2 * n_pairs), ("prim", 2 * n_pairs), ("sig", n_pairs), ("dup", n_pairs)):
        o[k] = o[k][:m]
    return rc, o


def index_from_device(lib, d_bwt, primary, L2, d_sa, d_pac, l_pac, ctg_off, ctg_len, sa_intv=32):
    """d_* are integer device addresses (e.g. torch.Tensor.data_ptr()); the caller keeps the tensors alive."""
    h = C.c_void_p()
    L2a = np.asarray(L2, dtype=np.uint64)
    co = np.asarray(ctg_off, dtype=np.int64)
    cl = np.asarray(ctg_len, dtype=np.int32)
    lib._chk(lib.l.ssg_index_from_device(C.c_void_p(d_bwt), C.c_uint64(primary), _ptr(L2a), C.c_void_p(d_sa), C.c_int(sa_intv),
                                         C.c_void_p(d_pac), C.c_int64(l_pac), C.c_int(len(co)), _ptr(co), _ptr(cl), C.byref(h)))
    return h


def hotpath_dev(lib, idx, opt, n_pairs, max_len, d_seq, d_off, d_pair_batch, n_batches=1, id0=0, want_dup=False):
    summary = np.zeros(8, dtype=np.uint64)
    dup = np.zeros(n_pairs, dtype=np.uint8) if want_dup else None
    lib._chk(lib.l.ssg_hotpath_dev(idx, _ptr(opt), C.c_int(n_pairs), C.c_int(max_len), C.c_void_p(d_seq), C.c_void_p(d_off), C.c_void_p(d_pair_batch),
                                   C.c_int(n_batches), C.c_int64(id0), _ptr(summary), _ptr(dup) if want_dup else None))
    return summary, dup


def hotpath_dev_ex(lib, idx, opt, n_pairs, max_len, d_seq, d_off, d_pair_batch, n_batches=1, id0=0, local_dedup=True, d_sig=None, keep=False):
    """ssg_hotpath_dev_ex: summary[16] (see include/ssgpu.h) and, with keep=True, the handle of the records left in HBM."""
    summary = np.zeros(16, dtype=np.uint64)
    h = C.c_void_p()
    lib._chk(lib.l.ssg_hotpath_dev_ex(idx, _ptr(opt), C.c_int(n_pairs), C.c_int(max_len), C.c_void_p(d_seq), C.c_void_p(d_off), C.c_void_p(d_pair_batch),
                                      C.c_int(n_batches), C.c_int64(id0), None, C.c_int(1 if local_dedup else 0), _ptr(summary), None,
                                      C.c_void_p(d_sig) if d_sig else None, C.byref(h) if keep else None))
    return summary, (h if keep else None)


def dev_records_classify(lib, h, d_dup):
    """samblaster's classification of kept records with externally decided duplicate flags (device pointer, one byte per pair)."""
    counts = np.zeros(4, dtype=np.uint64)
    lib._chk(lib.l.ssg_dev_records_classify(h, None, C.c_void_p(d_dup), _ptr(counts)))
    return counts


def markdup_sig_dev(lib, n, d_sig, d_ordinal, d_dup):
    """owner-side first-seen-wins over received signatures (device addresses): ssg_markdup_sig_dev"""
    lib._chk(lib.l.ssg_markdup_sig_dev(C.c_long(n), C.c_void_p(d_sig), C.c_void_p(d_ordinal), C.c_void_p(d_dup)))


def dev_records_n_lines(lib, h):
    lib.l.ssg_dev_records_n_lines.restype = C.c_int64
    return int(lib.l.ssg_dev_records_n_lines(h))


def dev_record_bytes(lib):
    lib.l.ssg_dev_record_bytes.restype = C.c_size_t
    return int(lib.l.ssg_dev_record_bytes())


def dev_records_export(lib, h, d_keys, d_recs=None, d_bits=None):
    """sort keys / fixed-size records / side-stream bits of the kept records into device buffers (addresses)"""
    lib._chk(lib.l.ssg_dev_records_export(h, C.c_void_p(d_keys), C.c_void_p(d_recs) if d_recs else None, C.c_void_p(d_bits) if d_bits else None))


def dev_records_download(lib, h, n_pairs):
    """records kept in HBM by hotpath_dev_ex(keep=True) -> (PeResult, per-line SSG_SBL_* bits, per-line mate line index)"""
    _bind_pe(lib)
    nl = dev_records_n_lines(lib, h)
    bits = np.zeros(nl, dtype=np.uint8)
    mate = np.zeros(nl, dtype=np.int64)
    r = C.c_void_p()
    lib._chk(lib.l.ssg_dev_records_download(h, C.byref(r), _ptr(bits), _ptr(mate)))
    return PeResult(lib, r, n_pairs, 0), bits, mate


def dev_records_free(lib, h):
    lib.l.ssg_dev_records_free(h)


def hotpath_dev_sig(lib, idx, opt, n_pairs, max_len, d_seq, d_off, d_pair_batch, d_sig, n_batches=1, id0=0):
    """hotpath_dev that also writes the pair signatures (device pointer d_sig: n_pairs x 3 uint64) for dist.global_markdup."""
    summary = np.zeros(8, dtype=np.uint64)
    lib._chk(lib.l.ssg_hotpath_dev_sig(idx, _ptr(opt), C.c_int(n_pairs), C.c_int(max_len), C.c_void_p(d_seq), C.c_void_p(d_off), C.c_void_p(d_pair_batch),
                                       C.c_int(n_batches), C.c_int64(id0), _ptr(summary), None, C.c_void_p(d_sig)))
    return summary, None


def prof_get(lib, cap=64):
    names = (C.c_char_p * cap)()
    ms = (C.c_double * cap)()
    cnt = (C.c_long * cap)()
    n = lib.l.ssg_prof_get(C.c_int(cap), names, ms, cnt)
    out = {}
    for i in range(min(n, cap)):   # the instance for reads up to 255 bases keeps the kernel's plain name; the other one says so
        k = names[i].decode().replace("<false>", "").replace("<true>", "<wide>").strip("()")
        a, b = out.get(k, (0.0, 0))
        out[k] = (a + ms[i], b + cnt[i])
    return out


def _bytes_u8(data):
    return np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)


def crc32_batch(lib, data, cut):
    """ssg_crc32_batch: zlib's CRC-32 of the byte ranges data[cut[i] .. cut[i+1]) (any length each), computed on the device."""
    data = _bytes_u8(data)
    cut = np.ascontiguousarray(cut, dtype=np.uint64)
    n = len(cut) - 1
    crc = np.zeros(max(n, 0), dtype=np.uint32)
    lib._chk(lib.l.ssg_crc32_batch(_ptr(data) if data.size else None, _ptr(cut), C.c_long(n), _ptr(crc)))
    return crc


def bgzf_bound(lib, payload_bytes, n_blocks):
    """ssg_bgzf_bound: an output capacity that always suffices for bgzf_compress (payload + 31 per block)."""
    lib.l.ssg_bgzf_bound.restype = C.c_uint64
    return int(lib.l.ssg_bgzf_bound(C.c_uint64(payload_bytes), C.c_long(n_blocks)))


def bgzf_deflate(lib, payload, cut, level=None):
    """ssg_bgzf_deflate (level None) / ssg_bgzf_deflate_level: the raw deflate stream of every block payload[cut[b] .. cut[b+1]).  Returns (out, out_off):
    block b's stream is out[out_off[b]:out_off[b+1]].  Levels 1..6 are the bytes of level None, 7..9 the chained match finder (csrc/k_bgzf_deep.h)."""
    payload = _bytes_u8(payload)
    cut = np.ascontiguousarray(cut, dtype=np.uint64)
    n = len(cut) - 1
    cap = (int(cut[-1] - cut[0]) if n > 0 else 0) + 5 * max(n, 0) + 64
    out = np.zeros(cap, dtype=np.uint8)
    off = np.zeros(max(n, 0) + 1, dtype=np.uint64)
    args = (_ptr(payload) if payload.size else None, _ptr(cut), C.c_long(n), _ptr(out), C.c_uint64(cap), _ptr(off))
    lib._chk(lib.l.ssg_bgzf_deflate(*args) if level is None else lib.l.ssg_bgzf_deflate_level(*args, C.c_int(level)))
    return out[:int(off[-1])], off


def bgzf_compress(lib, payload, cut, want_crc=True, out_cap=None, level=None):
    """ssg_bgzf_compress (level None) / ssg_bgzf_compress_level: the blocks payload[cut[b] .. cut[b+1]) (<= 0xff00 bytes each) as complete BGZF members, deflated,
    checksummed and framed on the device.  Returns (out, out_off, crc): member b is out[out_off[b]:out_off[b+1]], out[:out_off[-1]] a BGZF file's body; crc is None unless wanted."""
    payload = _bytes_u8(payload)
    cut = np.ascontiguousarray(cut, dtype=np.uint64)
    n = len(cut) - 1
    cap = bgzf_bound(lib, int(cut[-1] - cut[0]) if n > 0 else 0, n) if out_cap is None else int(out_cap)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    off = np.zeros(max(n, 0) + 1, dtype=np.uint64)
    crc = np.zeros(max(n, 1), dtype=np.uint32) if want_crc else None
    args = (_ptr(payload) if payload.size else None, _ptr(cut), C.c_long(n), _ptr(out), C.c_uint64(cap), _ptr(off), _ptr(crc) if want_crc else None)
    lib._chk(lib.l.ssg_bgzf_compress(*args) if level is None else lib.l.ssg_bgzf_compress_level(*args, C.c_int(level)))
    return out[:int(off[-1])], off, (crc[:max(n, 0)] if want_crc else None)


def bgzf_inflate(lib, members, moff, want_status=True, out_cap=None):
    """ssg_bgzf_inflate: the BGZF members members[moff[b] .. moff[b+1]) inflated and checksummed on the device.  Returns (rc, out, out_off, status):
    rc 0 or SSG_EIO (-5: status[] says which members are bad; 1 malformed, 2 length, 3 CRC-32), member b's bytes out[out_off[b]:out_off[b+1]];
    every other return code raises.  status is None unless wanted."""
    members = _bytes_u8(members)
    moff = np.ascontiguousarray(moff, dtype=np.uint64)
    n = len(moff) - 1
    if out_cap is None:
        out_cap = sum(int.from_bytes(members[int(e) - 4:int(e)].tobytes(), "little") for e in moff[1:] if int(e) >= 4) if n > 0 else 0
    out = np.zeros(max(int(out_cap), 1), dtype=np.uint8)
    off = np.zeros(max(n, 0) + 1, dtype=np.uint64)
    status = np.zeros(max(n, 1), dtype=np.int32) if want_status else None
    rc = lib.l.ssg_bgzf_inflate(_ptr(members) if members.size else None, _ptr(moff), C.c_long(n), _ptr(out), C.c_uint64(int(out_cap)), _ptr(off),
                                _ptr(status) if want_status else None)
    if rc != -5:
        lib._chk(rc)
    return rc, out[:int(off[-1])], off, (status[:max(n, 0)] if want_status else None)


class Recs:
    """A device-resident record store (ssg_recs_*): freed with the object or by close()."""

    def __init__(self, lib, h):
        self.lib, self.h = lib, h

    def close(self):
        if self.h is not None:
            self.lib.l.ssg_recs_free.argtypes = [C.c_void_p]
            self.lib.l.ssg_recs_free.restype = None
            self.lib.l.ssg_recs_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


def recs_create(lib, cap_bytes):
    """ssg_recs_create: a store on the calling thread's device for at most cap_bytes of chunks."""
    h = C.c_void_p()
    lib._chk(lib.l.ssg_recs_create(C.c_uint64(cap_bytes), C.byref(h)))
    return Recs(lib, h)


def recs_append(lib, recs, data):
    """ssg_recs_append: uploads one chunk of whole records; returns its id (the upper 24 bits of its records' locations)."""
    data = _bytes_u8(data)
    cid = C.c_uint32()
    lib._chk(lib.l.ssg_recs_append(recs.h, _ptr(data) if data.size else None, C.c_uint64(data.size), C.byref(cid)))
    return int(cid.value)


def recs_order(lib, recs, loc, cum):
    """ssg_recs_order: record i of the sorted stream lies at loc[i] = chunk << 40 | offset and occupies stream bytes cum[i] .. cum[i+1]."""
    loc = np.ascontiguousarray(loc, dtype=np.uint64)
    cum = np.ascontiguousarray(cum, dtype=np.uint64)
    assert len(cum) == len(loc) + 1
    lib._chk(lib.l.ssg_recs_order(recs.h, _ptr(loc) if loc.size else None, _ptr(cum), C.c_int64(len(loc))))


def recs_gather(lib, recs, v0, v1, out=None):
    """ssg_recs_gather: stream bytes v0 .. v1, gathered on the device (into out[:v1 - v0] if given)."""
    if out is None:
        out = np.zeros(max(int(v1) - int(v0), 1), dtype=np.uint8)
    lib._chk(lib.l.ssg_recs_gather(recs.h, C.c_uint64(v0), C.c_uint64(v1), _ptr(out)))
    return out[:max(int(v1) - int(v0), 0)]


def bgzf_compress_recs(lib, recs, cut, want_crc=True, out_cap=None, level=None):
    """ssg_bgzf_compress_recs (level None) / ssg_bgzf_compress_recs_level: bgzf_compress of the store's stream bytes cut[0] .. cut[-1] (absolute offsets), the payload gathered on the device."""
    cut = np.ascontiguousarray(cut, dtype=np.uint64)
    n = len(cut) - 1
    cap = bgzf_bound(lib, int(cut[-1] - cut[0]) if n > 0 else 0, n) if out_cap is None else int(out_cap)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    off = np.zeros(max(n, 0) + 1, dtype=np.uint64)
    crc = np.zeros(max(n, 1), dtype=np.uint32) if want_crc else None
    args = (recs.h, _ptr(cut), C.c_long(n), _ptr(out), C.c_uint64(cap), _ptr(off), _ptr(crc) if want_crc else None)
    lib._chk(lib.l.ssg_bgzf_compress_recs(*args) if level is None else lib.l.ssg_bgzf_compress_recs_level(*args, C.c_int(level)))
    return out[:int(off[-1])], off, (crc[:max(n, 0)] if want_crc else None)


BAM_ENT_DT = np.dtype([("tid", "i4"), ("pos", "i4"), ("end", "i4"), ("flag", "u4"), ("len", "u4"), ("pad", "u4")])
SSG_EALIGN = -71


def recs_append_bgzf(lib, recs, members, moff, want_status=True):
    """ssg_recs_append_bgzf: the BGZF members members[moff[b] .. moff[b+1]) inflated into a new chunk of the store.  Returns (rc, chunk_id, out_off, status):
    rc 0 or SSG_EIO (-5: a bad member, status[] says which; no chunk was added and chunk_id is None); every other return code raises."""
    members = _bytes_u8(members)
    moff = np.ascontiguousarray(moff, dtype=np.uint64)
    n = len(moff) - 1
    off = np.zeros(max(n, 0) + 1, dtype=np.uint64)
    status = np.zeros(max(n, 1), dtype=np.int32) if want_status else None
    cid = C.c_uint32(0xffffffff)
    rc = lib.l.ssg_recs_append_bgzf(recs.h, _ptr(members) if members.size else None, _ptr(moff), C.c_long(n), C.byref(cid), _ptr(off), _ptr(status) if want_status else None)
    if rc != -5:
        lib._chk(rc)
    return rc, (int(cid.value) if rc == 0 and n > 0 else None), off, (status[:max(n, 0)] if want_status else None)


def recs_scan(lib, recs, chunk_id, hint, first=0, cap=None):
    """ssg_recs_scan: the records of a chunk, found on the device.  hint: n_hints + 1 ascending offsets (the members' out_off).  Returns (rc, n_rec, loc, key, ent):
    rc 0, or SSG_EOVERFLOW (-75), SSG_EIO (-5), SSG_EALIGN (-71) with the arrays as the call left them (cap elements, prefilled with 0xAB bytes); every other
    return code raises.  ent has dtype BAM_ENT_DT."""
    hint = np.ascontiguousarray(hint, dtype=np.uint64)
    n_hints = len(hint) - 1
    if cap is None:
        cap = int(hint[-1]) // 36 if n_hints >= 0 and len(hint) else 0
    loc = np.full(cap + 1, 0xABABABABABABABAB, dtype=np.uint64)
    key = np.full(cap + 1, 0xABABABABABABABAB, dtype=np.uint64)
    ent = np.frombuffer(np.full((cap + 1) * BAM_ENT_DT.itemsize, 0xAB, dtype=np.uint8).tobytes(), dtype=BAM_ENT_DT).copy()
    n_rec = C.c_uint64(0)
    rc = lib.l.ssg_recs_scan(recs.h, C.c_uint32(chunk_id), _ptr(hint), C.c_int64(n_hints), C.c_uint64(first), C.c_uint64(cap), C.byref(n_rec), _ptr(loc), _ptr(key), _ptr(ent))
    if rc not in (0, -5, -75, SSG_EALIGN):
        lib._chk(rc)
    n = int(n_rec.value)
    if rc == 0:
        assert int(loc[cap]) == 0xABABABABABABABAB and int(key[cap]) == 0xABABABABABABABAB and ent[cap:].tobytes() == b"\xab" * BAM_ENT_DT.itemsize   # nothing behind cap
        return rc, n, loc[:n], key[:n], ent[:n]
    return rc, n, loc, key, ent


BAM_REGION_DT = np.dtype([("tid", "i4"), ("beg", "i4"), ("end", "i4")])
BAM_FOP_DT = np.dtype([("op", "u1"), ("arg", "u1"), ("pad", "u2"), ("value", "i4")])
FOP_MAX = 64
FOP_FLAG, FOP_AND, FOP_OR, FOP_NOT, FOP_EQ, FOP_NE, FOP_LT, FOP_LE, FOP_GT, FOP_GE = range(10)
FLD_MAPQ, FLD_REF_ID, FLD_MATE_REF_ID, FLD_TLEN, FLD_SEQ_LEN, FLD_FLAG = range(6)


def recs_select(lib, recs, chunk_id, hint, first=0, regions=(), prog=(), cap=None, counting=False):
    """ssg_recs_select: ssg_recs_scan with the decision taken on the device.  regions: (tid, beg, end) triples, 0-based half-open, sorted and disjoint; prog:
    (op, arg, value) triples of the postfix filter program.  Returns (rc, n_rec, n_sel, loc, key, ent) as recs_scan does, the arrays holding the kept records;
    counting=True is the counting form (cap 0, no arrays: loc, key and ent are None).  rc 0, SSG_EOVERFLOW (-75), SSG_EIO (-5), SSG_EALIGN (-71) or
    SSG_EINVAL (-22: the message is in ssg_last_error()); every other return code raises."""
    hint = np.ascontiguousarray(hint, dtype=np.uint64)
    n_hints = len(hint) - 1
    reg = np.array([tuple(x) for x in regions], dtype=BAM_REGION_DT)
    fop = np.array([(op, arg, 0, value) for op, arg, value in prog], dtype=BAM_FOP_DT)
    n_rec, n_sel = C.c_uint64(0), C.c_uint64(0)
    head = (recs.h, C.c_uint32(chunk_id), _ptr(hint), C.c_int64(n_hints), C.c_uint64(first), _ptr(reg) if len(reg) else None, C.c_int64(len(reg)),
            _ptr(fop) if len(fop) else None, C.c_int(len(fop)))
    if counting:
        rc = lib.l.ssg_recs_select(*head, C.c_uint64(0), C.byref(n_rec), C.byref(n_sel), None, None, None)
        if rc not in (0, -5, -22, -75, SSG_EALIGN):
            lib._chk(rc)
        return rc, int(n_rec.value), int(n_sel.value), None, None, None
    if cap is None:
        cap = int(hint[-1]) // 36 if n_hints >= 0 and len(hint) else 0
    loc = np.full(cap + 1, 0xABABABABABABABAB, dtype=np.uint64)
    key = np.full(cap + 1, 0xABABABABABABABAB, dtype=np.uint64)
    ent = np.frombuffer(np.full((cap + 1) * BAM_ENT_DT.itemsize, 0xAB, dtype=np.uint8).tobytes(), dtype=BAM_ENT_DT).copy()
    rc = lib.l.ssg_recs_select(*head, C.c_uint64(cap), C.byref(n_rec), C.byref(n_sel), _ptr(loc), _ptr(key), _ptr(ent))
    if rc not in (0, -5, -22, -75, SSG_EALIGN):
        lib._chk(rc)
    n = int(n_sel.value)
    if rc == 0:
        assert int(loc[cap]) == 0xABABABABABABABAB and int(key[cap]) == 0xABABABABABABABAB and ent[cap:].tobytes() == b"\xab" * BAM_ENT_DT.itemsize   # nothing behind cap
        return rc, int(n_rec.value), n, loc[:n], key[:n], ent[:n]
    return rc, int(n_rec.value), n, loc, key, ent


def device_memory(lib):
    """ssg_device_memory: (free, total) bytes of the calling thread's device."""
    f, t = C.c_uint64(0), C.c_uint64(0)
    lib._chk(lib.l.ssg_device_memory(C.byref(f), C.byref(t)))
    return int(f.value), int(t.value)


def recs_reopen(lib, recs):
    """ssg_recs_reopen: drops a declared order; the store takes appends again."""
    lib._chk(lib.l.ssg_recs_reopen(recs.h))


def recs_release(lib, recs, chunk_id):
    """ssg_recs_release: frees a chunk's device memory and returns its bytes to the capacity; the id stays taken."""
    lib._chk(lib.l.ssg_recs_release(recs.h, C.c_uint32(chunk_id)))


SSG_ERANGE = -34
B2F_RUN_MAX = 256


class B2f:
    """bamtofastq on a record store (ssg_b2f_*): freed with the object or by close(), before its store."""

    def __init__(self, lib, h, recs):
        self.lib, self.h, self.recs = lib, h, recs   # (the store is kept alive: the carry counts against it)

    def close(self):
        if self.h is not None:
            self.lib.l.ssg_b2f_free.argtypes = [C.c_void_p]
            self.lib.l.ssg_b2f_free.restype = None
            if self.recs.h is not None:
                self.lib.l.ssg_b2f_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


def b2f_create(lib, recs, rg=(), rename=False, hash_bits=64, raw=False):
    """ssg_b2f_create: rg is the -r list (bytes or str ids; None stands for a NULL id).  raw=True returns (rc, B2f or None) instead of raising."""
    ids = [None if x is None else (x if isinstance(x, bytes) else x.encode()) for x in rg]
    arr = (C.c_char_p * max(len(ids), 1))(*ids)
    h = C.c_void_p()
    rc = lib.l.ssg_b2f_create(recs.h if recs is not None else None, arr if ids else None, C.c_int(len(ids)), C.c_int(1 if rename else 0), C.c_int(hash_bits), C.byref(h))
    if raw:
        return rc, (B2f(lib, h, recs) if rc == 0 else None)
    lib._chk(rc)
    return B2f(lib, h, recs)


def b2f_push(lib, b, chunk_id, hint, first=0, out_cap=None):
    """ssg_b2f_push: returns (rc, text, out_len, n_rec, n_pairs).  out_cap None: the documented bound 2 * (hint[-1] + carried bytes) + 64.  No return code
    raises; text is the bytes written (b"" unless rc == 0), and the buffer behind them is seen to be untouched."""
    hint = np.ascontiguousarray(hint, dtype=np.uint64)
    n_hints = len(hint) - 1
    if out_cap is None:
        out_cap = 2 * ((int(hint[-1]) if len(hint) else 0) + b2f_waiting(lib, b)[1]) + 64
    out = np.full(int(out_cap) + 8, 0xAB, dtype=np.uint8)
    out_len, n_rec, n_pairs = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = lib.l.ssg_b2f_push(b.h, C.c_uint32(chunk_id), _ptr(hint) if len(hint) else None, C.c_int64(n_hints), C.c_uint64(first), _ptr(out), C.c_uint64(int(out_cap)),
                            C.byref(out_len), C.byref(n_rec), C.byref(n_pairs))
    n = int(out_len.value)
    if rc == 0:
        assert n <= out_cap and (out[n:] == 0xAB).all()             # nothing behind the text
        return rc, out[:n].tobytes(), n, int(n_rec.value), int(n_pairs.value)
    assert (out == 0xAB).all()                                       # a failure writes nothing
    return rc, b"", n, int(n_rec.value), int(n_pairs.value)


def b2f_waiting(lib, b):
    """ssg_b2f_waiting: (halves held, bytes of their records)."""
    n, by = C.c_uint64(0), C.c_uint64(0)
    lib._chk(lib.l.ssg_b2f_waiting(b.h, C.byref(n), C.byref(by)))
    return int(n.value), int(by.value)


DEPTH_THR_MAX = 8


class Depth:
    """coverage on a record store (ssg_depth_*): freed with the object or by close(), before its store."""

    def __init__(self, lib, h, recs):
        self.lib, self.h, self.recs = lib, h, recs

    def close(self):
        if self.h is not None:
            self.lib.l.ssg_depth_free.argtypes = [C.c_void_p]
            self.lib.l.ssg_depth_free.restype = None
            if self.recs.h is not None:
                self.lib.l.ssg_depth_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


def depth_create(lib, recs, prog=(), min_baseq=0):
    """ssg_depth_create: prog as recs_select takes it.  Returns (rc, Depth or None); no return code raises."""
    fop = np.array([(op, arg, 0, value) for op, arg, value in prog], dtype=BAM_FOP_DT)
    h = C.c_void_p()
    rc = lib.l.ssg_depth_create(recs.h if recs is not None else None, _ptr(fop) if len(fop) else None, C.c_int(len(fop)), C.c_int(min_baseq), C.byref(h))
    return rc, (Depth(lib, h, recs) if rc == 0 else None)


def depth_begin(lib, d, tid, beg, end):
    """ssg_depth_begin: opens the span [beg, end) of contig tid; the return code."""
    return lib.l.ssg_depth_begin(d.h, C.c_int32(tid), C.c_int64(beg), C.c_int64(end))


def depth_push(lib, d, chunk_id, hint, first=0):
    """ssg_depth_push: returns (rc, n_rec, n_used, n_later, descents, n_behind); no return code raises."""
    hint = np.ascontiguousarray(hint, dtype=np.uint64)
    n_hints = len(hint) - 1
    v = [C.c_uint64(0) for _ in range(5)]
    rc = lib.l.ssg_depth_push(d.h, C.c_uint32(chunk_id), _ptr(hint) if len(hint) else None, C.c_int64(n_hints), C.c_uint64(first), *[C.byref(x) for x in v])
    return (rc,) + tuple(int(x.value) for x in v)


def depth_finish(lib, d):
    return lib.l.ssg_depth_finish(d.h)


def depth_end(lib, d):
    return lib.l.ssg_depth_end(d.h)


def depth_get(lib, d, p0, p1):
    """ssg_depth_get: (rc, span, cov) of the reference positions [p0, p1), uint32 arrays."""
    n = max(p1 - p0, 0)
    span = np.full(n + 1, 0xABABABAB, dtype=np.uint32)
    cov = np.full(n + 1, 0xABABABAB, dtype=np.uint32)
    rc = lib.l.ssg_depth_get(d.h, C.c_int64(p0), C.c_int64(p1), _ptr(span), _ptr(cov))
    assert int(span[n]) == 0xABABABAB and int(cov[n]) == 0xABABABAB           # nothing behind the positions
    return rc, span[:n], cov[:n]


def depth_sums(lib, d, pairs, thr=()):
    """ssg_depth_sums: pairs of (beg, end) reference positions; returns (rc, out) with out[k] = (sum span, sum cov, positions with cov >= thr[0], ...) as uint64."""
    reg = np.ascontiguousarray(np.array(pairs, dtype=np.int64).reshape(-1, 2))
    t = np.ascontiguousarray(thr, dtype=np.uint32)
    out = np.full((len(reg), 2 + len(t)), 0xABABABABABABABAB, dtype=np.uint64)
    rc = lib.l.ssg_depth_sums(d.h, _ptr(reg) if len(reg) else None, C.c_int64(len(reg)), _ptr(t) if len(t) else None, C.c_int(len(t)), _ptr(out) if out.size else None)
    return rc, out


def depth_text(lib, d, name, p0, p1, all_positions=False, cap=None):
    """ssg_depth_text: returns (rc, text, len).  cap None: the sizing form first, then a buffer of exactly that size; cap 0 alone is the sizing form (text b"").
    The buffer behind the text is seen to be untouched, and on a failure the whole of it."""
    name = name if isinstance(name, bytes) else name.encode()
    n = C.c_uint64(0)
    if cap is None:
        rc = lib.l.ssg_depth_text(d.h, name, C.c_int64(p0), C.c_int64(p1), C.c_int(1 if all_positions else 0), None, C.c_uint64(0), C.byref(n))
        if rc:
            return rc, b"", int(n.value)
        cap = int(n.value)
    if cap == 0:
        rc = lib.l.ssg_depth_text(d.h, name, C.c_int64(p0), C.c_int64(p1), C.c_int(1 if all_positions else 0), None, C.c_uint64(0), C.byref(n))
        return rc, b"", int(n.value)
    out = np.full(int(cap) + 8, 0xAB, dtype=np.uint8)
    rc = lib.l.ssg_depth_text(d.h, name, C.c_int64(p0), C.c_int64(p1), C.c_int(1 if all_positions else 0), _ptr(out), C.c_uint64(int(cap)), C.byref(n))
    if rc == 0:
        assert int(n.value) <= cap and (out[int(n.value):] == 0xAB).all()
        return rc, out[:int(n.value)].tobytes(), int(n.value)
    assert (out == 0xAB).all()
    return rc, b"", int(n.value)


STATS_SCALARS = ("filtered", "secondary", "dup", "dup_len", "max_len", "total_len", "qcfail", "paired", "first", "last", "unmapped", "bases_mapped", "mq0", "single",
                 "paired_mapped", "proper", "anomalous", "mismatches", "bases_cigar", "sum_qual", "max_qual", "chk_names", "chk_reads", "chk_quals", "sorted")
STATS_N_SCALARS, STATS_NGC, STATS_NINDEL = 32, 200, 300


class StatsOpt(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("max_len", "n_isize", "cov_min", "cov_max", "cov_step", "span")]


def stats_opt(max_len=1024, n_isize=8000, cov_min=1, cov_max=1000, cov_step=1, span=0):
    return StatsOpt(max_len, n_isize, cov_min, cov_max, cov_step, span)


class Stats:
    """the QC tables on a record store (ssg_stats_*): freed with the object or by close(), before its store."""

    def __init__(self, lib, h, recs, opt):
        self.lib, self.h, self.recs, self.opt = lib, h, recs, opt
        lib.l.ssg_stats_ncov.restype = C.c_int64
        self.n_cov = int(lib.l.ssg_stats_ncov(C.byref(opt)))

    def close(self):
        if self.h is not None:
            self.lib.l.ssg_stats_free.argtypes = [C.c_void_p]
            self.lib.l.ssg_stats_free.restype = None
            if self.recs.h is not None:
                self.lib.l.ssg_stats_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


def stats_create(lib, recs, prog=(), opt=None):
    """ssg_stats_create: prog as recs_select takes it, opt a StatsOpt (stats_opt()).  Returns (rc, Stats or None); no return code raises."""
    fop = np.array([(op, arg, 0, value) for op, arg, value in prog], dtype=BAM_FOP_DT)
    opt = opt if opt is not None else stats_opt()
    h = C.c_void_p()
    rc = lib.l.ssg_stats_create(recs.h if recs is not None else None, _ptr(fop) if len(fop) else None, C.c_int(len(fop)), C.byref(opt), C.byref(h))
    return rc, (Stats(lib, h, recs, opt) if rc == 0 else None)


def stats_push(lib, s, chunk_id, hint, first=0):
    """ssg_stats_push: returns (rc, n_rec, descents); no return code raises."""
    hint = np.ascontiguousarray(hint, dtype=np.uint64)
    n_rec, desc = C.c_uint64(0), C.c_uint64(0)
    rc = lib.l.ssg_stats_push(s.h, C.c_uint32(chunk_id), _ptr(hint) if len(hint) else None, C.c_int64(len(hint) - 1), C.c_uint64(first), C.byref(n_rec), C.byref(desc))
    return rc, int(n_rec.value), int(desc.value)


def stats_finish(lib, s):
    return lib.l.ssg_stats_finish(s.h)


def stats_get(lib, s):
    """ssg_stats_get: (rc, dict) -- the scalars by name (STATS_SCALARS) and the tables quals[2][rows][256], bases[rows][6], gc[2][200], isize[3][n_isize], rl[rows],
    id[2][300], ic[4][rows], cov[n_cov] as uint64 arrays, rows = max_len + 1."""
    rows, ni = s.opt.max_len + 1, s.opt.n_isize
    shapes = {"quals": (2, rows, 256), "bases": (rows, 6), "gc": (2, STATS_NGC), "isize": (3, ni), "rl": (rows,), "id": (2, STATS_NINDEL), "ic": (4, rows), "cov": (s.n_cov,)}
    sc = np.zeros(STATS_N_SCALARS + 1, dtype=np.uint64)
    sc[STATS_N_SCALARS] = 0xABABABAB
    t = {k: np.full(int(np.prod(v)) + 1, 0xABABABAB, dtype=np.uint64) for k, v in shapes.items()}
    rc = lib.l.ssg_stats_get(s.h, _ptr(sc), *[_ptr(t[k]) for k in ("quals", "bases", "gc", "isize", "rl", "id", "ic", "cov")])
    assert int(sc[STATS_N_SCALARS]) == 0xABABABAB and all(int(a[-1]) == 0xABABABAB for a in t.values())   # nothing behind the tables
    out = {k: t[k][:-1].reshape(v) for k, v in shapes.items()}
    out.update({name: int(sc[i]) for i, name in enumerate(STATS_SCALARS)})
    return rc, out


MARKDUP_RUN_MAX = 256
MARKDUP_COUNTS = ("records", "taking_part", "paired", "pairs", "unmatched", "fragments", "dup_paired", "dup_fragments")
MARKDUP_N_COUNTS = 16


class Markdup:
    """the duplicate decision on a record store (ssg_markdup_*): freed with the object or by close(), before its store."""

    def __init__(self, lib, h, recs):
        self.lib, self.h, self.recs = lib, h, recs   # (the store is kept alive: the entries count against it)

    def close(self):
        if self.h is not None:
            self.lib.l.ssg_markdup_free.argtypes = [C.c_void_p]
            self.lib.l.ssg_markdup_free.restype = None
            if self.recs.h is not None:
                self.lib.l.ssg_markdup_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


def markdup_create(lib, recs, rg=(), lib_of_rg=(), hash_bits=64, n_rg=None):
    """ssg_markdup_create: rg the @RG ids (bytes or str; None stands for a NULL id), lib_of_rg their libraries; n_rg: another count than len(rg) (tests).
    Returns (rc, Markdup or None); no return code raises."""
    ids = [None if x is None else (x if isinstance(x, bytes) else x.encode()) for x in rg]
    arr = (C.c_char_p * max(len(ids), 1))(*ids)
    libs = np.ascontiguousarray(lib_of_rg, dtype=np.uint16)
    h = C.c_void_p()
    rc = lib.l.ssg_markdup_create(recs.h if recs is not None else None, arr if ids else None, _ptr(libs) if len(libs) else None, C.c_int(len(ids) if n_rg is None else n_rg),
                                  C.c_int(hash_bits), C.byref(h))
    return rc, (Markdup(lib, h, recs) if rc == 0 else None)


def markdup_push(lib, m, chunk_id, hint, first=0):
    """ssg_markdup_push: returns (rc, n_rec); no return code raises."""
    hint = np.ascontiguousarray(hint, dtype=np.uint64)
    n_rec = C.c_uint64(0)
    rc = lib.l.ssg_markdup_push(m.h, C.c_uint32(chunk_id), _ptr(hint) if len(hint) else None, C.c_int64(len(hint) - 1), C.c_uint64(first), C.byref(n_rec))
    return rc, int(n_rec.value)


def markdup_finish(lib, m):
    """ssg_markdup_finish: (rc, the counts by name (MARKDUP_COUNTS))."""
    c = np.zeros(MARKDUP_N_COUNTS + 1, dtype=np.uint64)
    c[MARKDUP_N_COUNTS] = 0xABABABAB
    rc = lib.l.ssg_markdup_finish(m.h, _ptr(c))
    assert int(c[MARKDUP_N_COUNTS]) == 0xABABABAB                       # nothing behind the counts
    return rc, {name: int(c[i]) for i, name in enumerate(MARKDUP_COUNTS)}


def markdup_get(lib, m, ord0, n):
    """ssg_markdup_get: (rc, the duplicate bits of ordinals ord0 .. ord0 + n as uint8)."""
    dup = np.full(max(int(n), 0) + 1, 0xAB, dtype=np.uint8)
    rc = lib.l.ssg_markdup_get(m.h, C.c_uint64(ord0), C.c_uint64(n), _ptr(dup))
    assert int(dup[-1]) == 0xAB                                          # nothing behind the bits
    return rc, dup[:-1]


def markdup_apply(lib, m, chunk_id, hint, first=0, remove=False, cap=None, counting=False):
    """ssg_markdup_apply: returns (rc, n_rec, n_kept, loc, ent), the arrays holding the kept records; counting=True is the counting form (cap 0, no arrays:
    loc and ent are None).  On a failure the arrays are as the call left them (cap elements, prefilled with 0xAB bytes).  No return code raises."""
    hint = np.ascontiguousarray(hint, dtype=np.uint64)
    n_hints = len(hint) - 1
    n_rec, n_kept = C.c_uint64(0), C.c_uint64(0)
    head = (m.h, C.c_uint32(chunk_id), _ptr(hint) if len(hint) else None, C.c_int64(n_hints), C.c_uint64(first), C.c_int(1 if remove else 0))
    if counting:
        rc = lib.l.ssg_markdup_apply(*head, C.c_uint64(0), C.byref(n_rec), C.byref(n_kept), None, None)
        return rc, int(n_rec.value), int(n_kept.value), None, None
    if cap is None:
        cap = int(hint[-1]) // 36 if n_hints >= 0 and len(hint) else 0
    loc = np.full(cap + 1, 0xABABABABABABABAB, dtype=np.uint64)
    ent = np.frombuffer(np.full((cap + 1) * BAM_ENT_DT.itemsize, 0xAB, dtype=np.uint8).tobytes(), dtype=BAM_ENT_DT).copy()
    rc = lib.l.ssg_markdup_apply(*head, C.c_uint64(cap), C.byref(n_rec), C.byref(n_kept), _ptr(loc), _ptr(ent))
    n = int(n_kept.value)
    assert int(loc[cap]) == 0xABABABABABABABAB and ent[cap:].tobytes() == b"\xab" * BAM_ENT_DT.itemsize   # nothing behind cap
    if rc == 0:
        return rc, int(n_rec.value), n, loc[:n], ent[:n]
    return rc, int(n_rec.value), n, loc, ent


def sam_format(lib, idx, opt, res, names, seq, off, quals=None, rg_id=""):
    n = 2 * res.n_pairs
    NA = (C.c_char_p * n)(*[s.encode() for s in names])
    QA = (C.c_char_p * n)(*[s.encode() for s in quals]) if quals is not None else None
    sam = C.c_char_p()
    sam_off = np.zeros(n + 1, dtype=np.int64)
    lib._chk(lib.l.ssg_sam_format(idx, _ptr(opt), res.h, C.c_int(res.n_pairs), NA, _ptr(seq), _ptr(off), QA, None, rg_id.encode(), C.byref(sam), _ptr(sam_off)))
    text = C.string_at(sam, int(sam_off[n])).decode()
    lib.l.ssg_free(sam)
    return text, sam_off


def bam_format(lib, idx, opt, res, names, seq, off, quals=None, rg_id=""):
    """ssg_bam_format: the host formatter's BAM records of a PeResult (what `sambamba view -S -f bam` makes of ssg_sam_format's lines)."""
    n = 2 * res.n_pairs
    NA = (C.c_char_p * n)(*[s.encode() for s in names])
    QA = (C.c_char_p * n)(*[(s.encode() if s is not None else None) for s in quals]) if quals is not None else None
    bam = C.c_void_p()
    bam_off = np.zeros(n + 1, dtype=np.int64)
    lib._chk(lib.l.ssg_bam_format(idx, _ptr(opt), res.h, C.c_int(res.n_pairs), NA, _ptr(seq), _ptr(off), QA, rg_id.encode(), C.byref(bam), _ptr(bam_off)))
    data = C.string_at(bam, int(bam_off[n]))
    lib.l.ssg_free(bam)
    return data, bam_off


BAM_CAND_DT = np.dtype([("pair", "i8"), ("first_rec", "i8"), ("n_rec", "i8"), ("byte_off", "i8"), ("n_bytes", "i8")])


def _take_pe_bam(lib, h, n_batches):
    l = lib.l
    for f in ("ssg_pe_bam_data", "ssg_pe_bam_cands", "ssg_pe_bam_pes", "ssg_pe_bam_stats"):
        getattr(l, f).restype = C.c_void_p
        getattr(l, f).argtypes = [C.c_void_p]
    for f in ("ssg_pe_bam_bytes", "ssg_pe_bam_n_rec", "ssg_pe_bam_n_cand"):
        getattr(l, f).restype = C.c_int64
        getattr(l, f).argtypes = [C.c_void_p]
    l.ssg_pe_bam_free.argtypes = [C.c_void_p]
    nb, nc = l.ssg_pe_bam_bytes(h), l.ssg_pe_bam_n_cand(h)
    out = {"bam": C.string_at(l.ssg_pe_bam_data(h), nb) if nb else b"", "n_rec": l.ssg_pe_bam_n_rec(h),
           "cands": np.frombuffer((C.c_char * (nc * BAM_CAND_DT.itemsize)).from_address(l.ssg_pe_bam_cands(h)), dtype=BAM_CAND_DT, count=nc).copy() if nc else np.zeros(0, BAM_CAND_DT),
           "pes": np.frombuffer((C.c_char * (n_batches * 4 * PESTAT_DT.itemsize)).from_address(l.ssg_pe_bam_pes(h)), dtype=PESTAT_DT, count=n_batches * 4).copy(),
           "stats": np.ctypeslib.as_array(C.cast(l.ssg_pe_bam_stats(h), C.POINTER(C.c_uint64)), shape=(8,)).copy()}
    l.ssg_pe_bam_free(h)
    return out


def mem_process_pairs_bam(lib, idx, opt, seq, off, names, quals=None, pair_batch=None, n_batches=1, id0=0, pes0=None, rg_id=""):
    """ssg_mem_process_pairs_bam: parsed reads in, BAM record bytes (made on the device) out."""
    n_pairs = (len(off) - 1) // 2
    n = 2 * n_pairs
    pair_batch = np.ascontiguousarray(pair_batch if pair_batch is not None else np.zeros(n_pairs, dtype=np.int32), dtype=np.int32)
    NA = (C.c_char_p * n)(*[s.encode() for s in names])
    QA = (C.c_char_p * n)(*[(s.encode() if s is not None else None) for s in quals]) if quals is not None else None
    h = C.c_void_p()
    p0 = _ptr(pes0) if pes0 is not None else None
    lib._chk(lib.l.ssg_mem_process_pairs_bam(idx, _ptr(opt), C.c_int(n_pairs), _ptr(seq), _ptr(off), NA, QA, _ptr(pair_batch), C.c_int(n_batches), C.c_int64(id0), p0,
                                             rg_id.encode() if rg_id else None, C.byref(h)))
    return _take_pe_bam(lib, h, n_batches)


def mem_process_fastq_bam(lib, idx, opt, text, rec_off, pair_batch=None, n_batches=1, id0=0, pes0=None, rg_id=""):
    """ssg_mem_process_fastq_bam: FASTQ text (bytes) of plain four-line records + the offset of every record's '@' in read order."""
    rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
    n_pairs = len(rec_off) // 2
    pair_batch = np.ascontiguousarray(pair_batch if pair_batch is not None else np.zeros(n_pairs, dtype=np.int32), dtype=np.int32)
    texts = [text] if isinstance(text, (bytes, bytearray)) else list(text)          # one piece, or several (the input files of a batch)
    bufs = [np.frombuffer(t, dtype=np.uint8) for t in texts]
    PA = (C.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs])
    nbytes = np.array([len(t) for t in texts], dtype=np.int64)
    h = C.c_void_p()
    p0 = _ptr(pes0) if pes0 is not None else None
    lib._chk(lib.l.ssg_mem_process_fastq_bam(idx, _ptr(opt), C.c_int(n_pairs), PA, _ptr(nbytes), C.c_int(len(bufs)), _ptr(rec_off), _ptr(pair_batch), C.c_int(n_batches),
                                             C.c_int64(id0), p0, rg_id.encode() if rg_id else None, C.byref(h)))
    return _take_pe_bam(lib, h, n_batches)
