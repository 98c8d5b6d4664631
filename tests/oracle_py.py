"""ctypes binding of the CPU oracle (oracle/liboracle.so) -- TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module.
"""
import ctypes as C

import numpy as np

from speedseq_amd.capi import ALN_DT, ALNREG_DT, ALNREQ_DT, INTV_DT


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Oracle:
    def __init__(self, so):
        self.l = C.CDLL(so)
        self.l.orc_idx_load.restype = C.c_void_p
        self.l.orc_idx_load.argtypes = [C.c_char_p]
        self.l.orc_idx_build_fasta.restype = C.c_void_p
        self.l.orc_idx_build_fasta.argtypes = [C.c_char_p]
        self.l.orc_idx_save.argtypes = [C.c_void_p, C.c_char_p]
        self.l.orc_idx_destroy.argtypes = [C.c_void_p]
        self.l.orc_api_opt_new.restype = C.c_void_p
        self.l.orc_api_align1_batch.restype = C.c_int64
        self.opt = C.c_void_p(self.l.orc_api_opt_new())

    def idx_load(self, prefix):
        h = self.l.orc_idx_load(prefix.encode())
        if not h:
            raise RuntimeError("oracle: cannot load index " + prefix)
        return C.c_void_p(h)

    def idx_build(self, fasta, save=True):
        h = self.l.orc_idx_build_fasta(fasta.encode())
        if not h:
            raise RuntimeError("oracle: cannot build index from " + fasta)
        h = C.c_void_p(h)
        if save:
            assert self.l.orc_idx_save(h, fasta.encode()) == 0
        return h

    def extend2(self, q, t, w, end_bonus, zdrop, h0, opt=None):
        out = (C.c_int * 6)()
        self.l.orc_api_extend2(opt or self.opt, C.c_int(len(q)), _ptr(q), C.c_int(len(t)), _ptr(t), C.c_int(w), C.c_int(end_bonus), C.c_int(zdrop), C.c_int(h0), out)
        return tuple(out)

    def opt_scores(self, a, b, o_del, e_del, o_ins, e_ins):
        """an option block of its own with this scoring (release: let it go)"""
        o = C.c_void_p(self.l.orc_api_opt_new())
        self.l.orc_api_opt_scores(o, C.c_int(a), C.c_int(b), C.c_int(o_del), C.c_int(e_del), C.c_int(o_ins), C.c_int(e_ins))
        return o

    def opt_chain(self, drop_ratio, mask_level, min_chain_weight, max_chain_extend, max_chain_gap):
        """an option block of its own with these chain-filter settings"""
        o = C.c_void_p(self.l.orc_api_opt_new())
        self.l.orc_api_opt_chain(o, C.c_float(drop_ratio), C.c_float(mask_level), C.c_int(min_chain_weight), C.c_int(max_chain_extend), C.c_int(max_chain_gap))
        return o

    def opt_seed(self, min_seed_len, split_factor, split_width, max_occ, max_mem_intv):
        """an option block of its own with these seeding settings"""
        o = C.c_void_p(self.l.orc_api_opt_new())
        self.l.orc_api_opt_seed(o, C.c_int(min_seed_len), C.c_float(split_factor), C.c_int(split_width), C.c_int(max_occ), C.c_int64(max_mem_intv))
        return o

    def align2(self, q, t, xtra, opt=None):
        out = (C.c_int * 7)()
        self.l.orc_api_align2(opt or self.opt, C.c_int(len(q)), _ptr(q), C.c_int(len(t)), _ptr(t), C.c_int(xtra), out)
        return tuple(out)

    def global2(self, q, t, w, cap=64, opt=None):
        n = C.c_int(0)
        cig = np.zeros(cap, dtype=np.uint32)
        sc = self.l.orc_api_global2(opt or self.opt, C.c_int(len(q)), _ptr(q), C.c_int(len(t)), _ptr(t), C.c_int(w), C.byref(n), _ptr(cig), C.c_int(cap))
        return sc, n.value, cig

    def collect_intv(self, idx, seq, cap=4096, opt=None):
        out = np.zeros(cap, dtype=INTV_DT)
        n = self.l.orc_api_collect_intv(opt or self.opt, idx, C.c_int(len(seq)), _ptr(seq), _ptr(out), C.c_int(cap))
        return out[:n]

    def seeds(self, idx, seq, cap=1 << 16, opt=None):
        """(rbeg, qbeg, len, rid) of every seed mem_chain visits for the read, in its order"""
        out = np.zeros((cap, 4), dtype=np.int64)
        self.l.orc_api_seeds.restype = C.c_int64
        n = self.l.orc_api_seeds(opt or self.opt, idx, C.c_int(len(seq)), _ptr(seq), _ptr(out), C.c_int64(cap))
        assert n <= cap
        return out[:n]

    def opt_chain2(self, opt, w, min_seed_len, max_occ):
        """the remaining knobs of the chaining stage on an option block of opt_chain()"""
        self.l.orc_api_opt_chain2(opt, C.c_int(w), C.c_int(min_seed_len), C.c_int(max_occ))
        return opt

    def chain(self, l_pac, read_len, seed_off, seeds4, intv_off, intv, opt=None, kbtree=1):
        """the chaining stage on given seeds ((rbeg, qbeg, len, rid) rows) and intervals (orc_api_chain): (chain_off, rows (pos, rid, n, w, kept, frac_rep bits, offset of
        the seed indices) of the chains as mem_chain_flt leaves them after its sort -- kept = 0 included --, seed indices counted from the read's first seed)"""
        read_len = np.ascontiguousarray(read_len, dtype=np.int32)
        seed_off = np.ascontiguousarray(seed_off, dtype=np.int64)
        intv_off = np.ascontiguousarray(intv_off, dtype=np.int64)
        seeds4 = np.ascontiguousarray(seeds4, dtype=np.int64).reshape(-1, 4)
        intv = np.ascontiguousarray(intv, dtype=INTV_DT)
        n, tot = len(read_len), int(seed_off[-1])
        assert len(seed_off) == n + 1 and len(intv_off) == n + 1 and len(seeds4) >= tot and len(intv) >= intv_off[-1]
        chain_off = np.zeros(n + 1, dtype=np.int64)
        chains = np.zeros((tot + 1, 7), dtype=np.int64)
        cseeds = np.zeros(tot + 1, dtype=np.int32)
        self.l.orc_api_set_chain_container(C.c_int(kbtree))
        self.l.orc_api_chain(opt or self.opt, C.c_int64(l_pac), C.c_int(n), _ptr(read_len), _ptr(seed_off), _ptr(seeds4), _ptr(intv_off), _ptr(intv),
                             _ptr(chain_off), _ptr(chains), _ptr(cseeds))
        self.l.orc_api_set_chain_container(C.c_int(-1))   # back to "not chosen": the next call on this thread chooses as before
        nc =int(chain_off[n])
        return chain_off, chains[:nc], cseeds[:int(chains[:nc, 2].sum())]

    def opt_regions(self, opt, w, zdrop, pen_clip5, pen_clip3, max_chain_gap, mask_level_redun):
        """the knobs of the region stage on an option block of opt_scores()"""
        self.l.orc_api_opt_regions(opt, C.c_int(w), C.c_int(zdrop), C.c_int(pen_clip5), C.c_int(pen_clip3), C.c_int(max_chain_gap), C.c_float(mask_level_redun))
        return opt

    def regions(self, pac, l_pac, ctg_off, ctg_len, seq, off, seed_off, seeds4, chain_off, chains3, chain_seeds, opt=None):
        """the region stage on given chains (orc_api_regions): seeds as (rbeg, qbeg, len, unused) rows, chains as (rid, n, frac_rep bits) rows with their seed indices
        one after another in chain_seeds: (reg_off, regions [ALNREG_DT], regions per read before mem_sort_dedup_patch)"""
        pac = np.ascontiguousarray(pac, dtype=np.uint8)
        ctg_off = np.ascontiguousarray(ctg_off, dtype=np.int64)
        ctg_len = np.ascontiguousarray(ctg_len, dtype=np.int32)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        seed_off = np.ascontiguousarray(seed_off, dtype=np.int64)
        chain_off = np.ascontiguousarray(chain_off, dtype=np.int64)
        seeds4 = np.ascontiguousarray(seeds4, dtype=np.int64).reshape(-1, 4)
        chains3 = np.ascontiguousarray(chains3, dtype=np.int64).reshape(-1, 3)
        chain_seeds = np.ascontiguousarray(chain_seeds, dtype=np.int32)
        n = len(off) - 1
        assert len(pac) >= l_pac // 4 + 1 and len(seed_off) == n + 1 and len(chain_off) == n + 1 and len(seeds4) >= seed_off[-1] and len(chains3) >= chain_off[-1]
        assert len(chain_seeds) >= int(chains3[:int(chain_off[-1]), 1].sum())
        reg_off, n_before = np.zeros(n + 1, dtype=np.int64), np.zeros(n, dtype=np.int32)
        cap = int(seed_off[-1]) + 1
        out = np.zeros(cap, dtype=ALNREG_DT)
        self.l.orc_api_regions.restype = C.c_int64
        tot = self.l.orc_api_regions(opt or self.opt, _ptr(pac), C.c_int64(l_pac), C.c_int(len(ctg_off)), _ptr(ctg_off), _ptr(ctg_len), C.c_int(n), _ptr(seq), _ptr(off),
                                     _ptr(seed_off), _ptr(seeds4), _ptr(chain_off), _ptr(chains3), _ptr(chain_seeds), _ptr(reg_off), _ptr(out), C.c_int64(cap), _ptr(n_before))
        assert tot <= cap
        return reg_off, out[:tot], n_before

    def align1_batch(self, idx, seq, off, opt=None):
        n = len(off) - 1
        reg_off = np.zeros(n + 1, dtype=np.int64)
        cap = 64 * n + 1024
        while True:
            out = np.zeros(cap, dtype=ALNREG_DT)
            tot = self.l.orc_api_align1_batch(opt or self.opt, idx, C.c_int(n), _ptr(seq), _ptr(off), _ptr(reg_off), _ptr(out), C.c_int64(cap))
            if tot <= cap:
                return reg_off, out[:tot]
            cap = tot

    def pestat(self, idx, reg_off, regs, pair_batch, n_batches, opt=None):
        """orc_mem_pestat on given region lists, per batch: n_batches x 4 models (PESTAT_DT)"""
        from speedseq_amd.capi import PESTAT_DT
        reg_off = np.ascontiguousarray(reg_off, dtype=np.int64)
        regs = np.ascontiguousarray(regs, dtype=ALNREG_DT)
        pair_batch = np.ascontiguousarray(pair_batch, dtype=np.int32)
        pes = np.zeros(4 * n_batches, dtype=PESTAT_DT)
        self.l.orc_api_pestat(opt or self.opt, idx, C.c_int((len(reg_off) - 1) // 2), _ptr(reg_off), _ptr(regs), _ptr(pair_batch), C.c_int(n_batches), _ptr(pes))
        return pes

    def reg2aln(self, pac, l_pac, ctg_off, ctg_len, seq, off, regs, req, opt=None):
        """the record stage on given regions [ALNREG_DT] and requests [ALNREQ_DT] (orc_api_reg2aln): (records [ALN_DT], per record 1 where upstream's CIGAR or MD
        is beyond the layout's capacity and was cut).  The caller validates: orc_mem_reg2aln trusts its region."""
        pac = np.ascontiguousarray(pac, dtype=np.uint8)
        ctg_off = np.ascontiguousarray(ctg_off, dtype=np.int64)
        ctg_len = np.ascontiguousarray(ctg_len, dtype=np.int32)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        regs = np.ascontiguousarray(regs, dtype=ALNREG_DT)
        req = np.ascontiguousarray(req, dtype=ALNREQ_DT)
        assert len(pac) >= l_pac // 4 + 1 and len(seq) >= off[-1]
        assert all(0 <= int(r["read"]) < len(off) - 1 and int(r["reg"]) < len(regs) for r in req)
        out, over = np.zeros(len(req) + 1, dtype=ALN_DT), np.zeros(len(req) + 1, dtype=np.uint8)
        self.l.orc_api_reg2aln.restype = C.c_int64
        self.l.orc_api_reg2aln(opt or self.opt, _ptr(pac), C.c_int64(l_pac), C.c_int(len(ctg_off)), _ptr(ctg_off), _ptr(ctg_len), C.c_int(len(off) - 1), _ptr(seq), _ptr(off),
                               C.c_int64(len(regs)), _ptr(regs), C.c_int64(len(req)), _ptr(req), _ptr(out), _ptr(over))
        return out[:len(req)], over[:len(req)]

    def pair_final(self, idx, id0, reg_off, regs, pes, opt=None):
        """primary marking, pairing and mem_sam_pe's decision on given region lists: (regions as the stage leaves them, req_off, records as
        (kind, reg, owner, flag, mapq) rows)"""
        reg_off = np.ascontiguousarray(reg_off, dtype=np.int64)
        regs = np.ascontiguousarray(regs, dtype=ALNREG_DT)
        pes = np.ascontiguousarray(pes)
        n = len(reg_off) - 1
        out = np.zeros(len(regs), dtype=ALNREG_DT)
        req_off = np.zeros(n + 1, dtype=np.int64)
        req = np.zeros((2 * len(regs) + n + 1, 5), dtype=np.int32)
        self.l.orc_api_pair_final(opt or self.opt, idx, C.c_int(n // 2), C.c_int64(id0), _ptr(reg_off), _ptr(regs), _ptr(pes), _ptr(out), _ptr(req_off), _ptr(req))
        return out, req_off, req[:req_off[n]]

    def chain_exposure(self, idx, seq, off, n_threads=8, opt=None, per_read=False):
        """every read through both containers of mem_chain (orc_mem.c: the position-sorted array the kernels restate, and klib's B-tree as upstream uses it):
        dict(differ, gt9_and_dup, gt9, dup, reads) [+ per-read flags]"""
        n = len(off) - 1
        out = np.zeros(5, dtype=np.int64)
        which = np.zeros(n, dtype=np.int32) if per_read else None
        self.l.orc_api_chain_exposure(opt or self.opt, idx, C.c_int(n), _ptr(seq), _ptr(off), C.c_int(n_threads), _ptr(out), _ptr(which) if per_read else None)
        d = dict(differ=int(out[0]), gt9_and_dup=int(out[1]), gt9=int(out[2]), dup=int(out[3]), reads=int(out[4]))
        return (d, which) if per_read else d

    def lazyf(self, on=-1):
        """(calls, calls that differ) of orc_ksw_align2 under the lazy-F exposure count; on = 1 / 0 switches the counting on / off, -1 only reads"""
        out = np.zeros(2, dtype=np.uint64)
        self.l.orc_api_lazyf(C.c_int(on), _ptr(out))
        return int(out[0]), int(out[1])

    def samblaster(self, sam_text, exclude_dups=True, add_mate_tags=True, max_split=2, min_non_overlap=20):
        """Oracle samblaster over SAM text (via temp files); returns the marked SAM text."""
        import os
        import subprocess
        import tempfile
        exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "orc_bwa")
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "in.sam"), "w") as f:
                f.write(sam_text)
            cmd = [exe, "samblaster"] + (["--excludeDups"] if exclude_dups else []) + (["--addMateTags"] if add_mate_tags else []) + \
                  ["--maxSplitCount", str(max_split), "--minNonOverlap", str(min_non_overlap),
                   "--splitterFile", os.path.join(d, "spl.sam"), "--discordantFile", os.path.join(d, "disc.sam")]
            with open(os.path.join(d, "in.sam")) as fi:
                out = subprocess.run(cmd, stdin=fi, capture_output=True, text=True, check=True).stdout
            self.last_splitters = open(os.path.join(d, "spl.sam")).read()
            self.last_discordants = open(os.path.join(d, "disc.sam")).read()
        return out

    def process_pairs(self, idx, seq, off, names, quals=None, n_processed=0, rg_id="", n_threads=1, pes0=None):
        from speedseq_amd.capi import PESTAT_DT
        n = len(off) - 1
        NA = (C.c_char_p * n)(*[s.encode() for s in names])
        QA = (C.c_char_p * n)(*[s.encode() for s in quals]) if quals is not None else None
        pes = np.zeros(4, dtype=PESTAT_DT)
        sam_off = np.zeros(n + 1, dtype=np.int64)
        self.l.orc_api_process_pairs.restype = C.c_void_p
        p = self.l.orc_api_process_pairs(self.opt, idx, C.c_int(n // 2), _ptr(seq), _ptr(off), NA, QA, C.c_int64(n_processed), rg_id.encode(),
                                         C.c_int(n_threads), _ptr(pes0) if pes0 is not None else None, _ptr(pes), _ptr(sam_off))
        text = C.string_at(p, int(sam_off[n])).decode()
        self.l.orc_api_free(C.c_void_p(p))
        return text, sam_off, pes
