"""What the seven stage test entries (ssg_dbg_chain, ssg_dbg_regions, ssg_dbg_reg2aln, ssg_dbg_pestat, ssg_dbg_pair_final, ssg_dbg_matesw, ssg_dbg_sbl_records) answer to malformed
input: the return code AND the whole message, and which refusal wins where two apply.  The reference tests of the stages mostly ask for "-22" alone; the strings
below were taken from the library as it stood before the entries moved into a translation unit of their own, so a message or an order of checks that changes with
such a move fails here.

Every case is one change to a valid call of the smallest shape (two reads of 100 and 80 bases copied from a two-contig reference, three seeds, two chains, two
regions, two requests; the pairing entries on the bundled example index); the valid call itself must succeed.  No refusal below starts a stage's kernels: the only
device work a refused call may do is the entry's uploads and its work order (the -w cases of ssg_dbg_regions).

Literals of the entries' source, counted by hand (each `bad = "..."` and each direct `ssg_err_msg = "ssg_dbg_..."`):
  ssg_dbg_chain      9 bad + 5 direct   reached: 9 + 1
  ssg_dbg_regions   14 bad + 5 direct   reached: 14 + 3
  ssg_dbg_reg2aln   13 bad + 2 direct   reached: 13 + 2
  dbg_check_regs     9 bad              reached: 9, through each of the three pairing entries
  ssg_dbg_pestat     2 direct           reached: 2
  ssg_dbg_pair_final 1 direct           reached: 1
  ssg_dbg_matesw     4 direct           reached: 4 (and its unprefixed "reads longer than 310 bases ...")
  ssg_dbg_sbl_records 6 refusals + 2 direct  reached: 6 + 1 (and the unprefixed "samblaster: --maxSplitCount above 16 ..."; not "n_pairs < 2^31": 2^32 offsets)
plus the scoring limits the entries call (check_band, check_scores, check_gap_penalties: 4 messages).  Not reachable by any input a test can hold: "more than 2^31
seeds" of chain and regions (every read has fewer than 2^24 seeds and each is read by the validator: 48 GB of seeds), and the four SSG_EOVERFLOW messages about
counts "outside its slice", which only a kernel that wrote nonsense could cause.
"""
import ctypes as C

import numpy as np
import pytest

import common
from speedseq_amd import capi
from speedseq_amd.capi import _ptr

EINVAL = -22
L0, L1 = 40000, 30000                    # two contigs; above 32768 bases so that a region can be too long without leaving its strand
L_PAC, CTG_OFF, CTG_LEN = L0 + L1, [0, L0], [L0, L1]
TEXT = np.random.RandomState(20261020).randint(0, 4, L_PAC).astype(np.uint8)
PAC = np.zeros(L_PAC // 4 + 1, np.uint8)
for _k in range(4):
    PAC[:len(TEXT[_k::4])] |= TEXT[_k::4] << ((3 - _k) * 2)
SEQ = np.concatenate([TEXT[1000:1100], TEXT[L0 + 3500:L0 + 3580]])
OFF = np.array([0, 100, 180], np.int64)


def ch(a, field, value, k=0):
    b = a.copy()
    if field is None:
        b[k] = value
    else:
        b[field][k] = value
    return b


def i64(*v):
    return np.array(v, np.int64)


def opt_with(lib, **kw):
    o = lib.opt_init()
    for k, v in kw.items():
        o[k] = v
    return o


def answer(lib, rc):
    return (rc, lib.l.ssg_last_error().decode() if rc else "")


def base_seeds():
    seeds = np.zeros(3, capi.SEED_DT)
    seeds["rbeg"], seeds["qbeg"], seeds["len"] = [1010, 1040, L0 + 3505], [10, 40, 5], [20, 20, 25]
    return seeds


# ------------------------------------------------------------------------------------------------------------------------------
# the entries, called as they are (the wrappers of capi.py assert what some of these cases break)
# ------------------------------------------------------------------------------------------------------------------------------
def base_chain():
    intv = np.zeros(3, capi.INTV_DT)
    intv["info"], intv["x2"] = [10 << 32 | 30, 40 << 32 | 60, 5 << 32 | 30], 1
    return dict(l_pac=L_PAC, n_ctg=2, n_reads=2, read_len=np.array([100, 80], np.int32), seed_off=i64(0, 2, 3), seeds=base_seeds(), rids=np.array([0, 0, 1], np.int32),
                intv_off=i64(0, 2, 3), intv=intv)


def call_chain(lib, a):
    n = max(a["n_reads"], 0)
    chain_off, form, cp, sp = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int32), C.c_void_p(), C.c_void_p()
    rc = lib.l.ssg_dbg_chain(_ptr(a["opt"]), C.c_int64(a["l_pac"]), C.c_int(a["n_ctg"]), C.c_int(a["n_reads"]), _ptr(a["read_len"]), _ptr(a["seed_off"]), _ptr(a["seeds"]), _ptr(a["rids"]),
                             _ptr(a["intv_off"]), _ptr(a["intv"]), _ptr(chain_off), C.byref(cp), C.byref(sp), _ptr(form))
    lib.l.ssg_free(cp); lib.l.ssg_free(sp)
    return answer(lib, rc)


def base_regions():
    chains = np.zeros(2, capi.CHAIN_DT)
    chains["n"], chains["first_seed"], chains["rid"], chains["frac_rep"] = [2, 1], [0, 2], [0, 1], 0.25
    return dict(l_pac=L_PAC, ctg_off=i64(*CTG_OFF), ctg_len=np.array(CTG_LEN, np.int32), n_reads=2, seq=SEQ, off=OFF, seed_off=i64(0, 2, 3), seeds=base_seeds(), chain_off=i64(0, 1, 2),
                chains=chains, cs=np.array([0, 1, 0], np.int32))


def call_regions(lib, a):
    n = max(a["n_reads"], 0)
    reg_off, route, rp = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int32), C.c_void_p()
    rc = lib.l.ssg_dbg_regions(_ptr(a["opt"]), _ptr(PAC), C.c_int64(a["l_pac"]), C.c_int(len(a["ctg_off"])), _ptr(a["ctg_off"]), _ptr(a["ctg_len"]), C.c_int(a["n_reads"]), _ptr(a["seq"]),
                               _ptr(a["off"]), _ptr(a["seed_off"]), _ptr(a["seeds"]), _ptr(a["chain_off"]), _ptr(a["chains"]), _ptr(a["cs"]), _ptr(reg_off), C.byref(rp), _ptr(route))
    lib.l.ssg_free(rp)
    return answer(lib, rc)


def base_reg2aln():
    regs = np.zeros(2, capi.ALNREG_DT)
    regs["rb"], regs["re"], regs["qe"], regs["rid"] = [1000, L0 + 3500], [1100, L0 + 3580], [100, 80], [0, 1]
    regs["score"] = regs["truesc"] = [100, 80]
    regs["w"], regs["secondary"], regs["secondary_all"], regs["seedcov"], regs["sub_n"], regs["seedlen0"], regs["frac_rep"] = 100, -1, -1, 7, 1, 19, 0.25
    req = np.zeros(2, capi.ALNREQ_DT)
    req["read"], req["reg"], req["mapq"] = [0, 1], [0, 1], 37
    return dict(l_pac=L_PAC, ctg_off=i64(*CTG_OFF), ctg_len=np.array(CTG_LEN, np.int32), n_reads=2, seq=SEQ, off=OFF, n_regs=2, regs=regs, n_req=2, req=req)


def call_reg2aln(lib, a):
    alns, route, err = np.zeros(len(a["req"]) + 1, capi.ALN_DT), np.zeros(len(a["req"]) + 1, np.int32), C.c_int32(0)
    rc = lib.l.ssg_dbg_reg2aln(_ptr(a["opt"]), _ptr(PAC), C.c_int64(a["l_pac"]), C.c_int(len(a["ctg_off"])), _ptr(a["ctg_off"]), _ptr(a["ctg_len"]), C.c_int(a["n_reads"]), _ptr(a["seq"]),
                               _ptr(a["off"]), C.c_int64(a["n_regs"]), _ptr(a["regs"]), C.c_int64(a["n_req"]), _ptr(a["req"]), _ptr(alns), _ptr(route), C.byref(err))
    return answer(lib, rc)


_IDX = {}


def example_index(lib):
    """the bundled example index, loaded once per library: (handle, l_pac, n_ctg)"""
    if lib.path not in _IDX:
        idx = lib.index_load(common.EXAMPLE_FA)
        lib.l.ssg_index_n_ctg.argtypes = [type(idx)]
        _IDX[lib.path] = (idx, int(lib.l.ssg_index_l_pac(idx)), int(lib.l.ssg_index_n_ctg(idx)))
    return _IDX[lib.path]


def base_pair(lib):
    """one pair as tests/test_pair_reference.py lays its simplest one out: a forward region at 1000 and its mate 400 bases on, reverse"""
    idx, L, n_ctg = example_index(lib)
    regs = np.zeros(2, capi.ALNREG_DT)
    regs["rb"], regs["re"], regs["qe"] = [1000, 2 * L - 1401], [1100, 2 * L - 1301], 100
    regs["score"] = regs["truesc"] = 100
    regs["seedcov"], regs["w"], regs["seedlen0"] = 50, 100, 19
    pes = np.zeros(4, capi.PESTAT_DT)
    pes["failed"] = 1
    pes[1] = (100, 700, 0, 0, 400.0, 50.0)
    seq = np.random.RandomState(7).randint(0, 4, 200).astype(np.uint8)
    return dict(idx=idx, n_pairs=1, reg_off=i64(0, 1, 2), regs=regs, pes=pes, pair_batch=np.zeros(1, np.int32), n_batches=1, seq=seq, read_off=i64(0, 100, 200))


def call_pestat(lib, a):
    out = np.zeros(4 * 64, capi.PESTAT_DT)
    return answer(lib, lib.l.ssg_dbg_pestat(a["idx"], _ptr(a["opt"]), C.c_int(a["n_pairs"]), _ptr(a["reg_off"]), _ptr(a["regs"]), _ptr(a["pair_batch"]), C.c_int(a["n_batches"]), _ptr(out)))


def call_pair_final(lib, a):
    out, req_off, rp = np.zeros(len(a["regs"]) + 1, capi.ALNREG_DT), np.zeros(4, np.int64), C.c_void_p()
    rc = lib.l.ssg_dbg_pair_final(a["idx"], _ptr(a["opt"]), C.c_int(a["n_pairs"]), C.c_int64(0), _ptr(a["reg_off"]), _ptr(a["regs"]), _ptr(a["pes"]), _ptr(out), _ptr(req_off), C.byref(rp))
    lib.l.ssg_free(rp)
    return answer(lib, rc)


def call_matesw(lib, a):
    out_off, n_out, err, counts, rp = np.zeros(4, np.int64), np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(8, np.uint64), C.c_void_p()
    rc = lib.l.ssg_dbg_matesw(a["idx"], _ptr(a["opt"]), C.c_int(a["n_pairs"]), _ptr(a["seq"]), _ptr(a["read_off"]), _ptr(a["reg_off"]), _ptr(a["regs"]), None, _ptr(a["pes"]),
                              C.c_int(-1), _ptr(out_off), C.byref(rp), _ptr(n_out), _ptr(err), _ptr(counts))
    lib.l.ssg_free(rp)
    return answer(lib, rc)


# ------------------------------------------------------------------------------------------------------------------------------
# the cases: (what is changed, the answer's text without the entry's name in front; None = accepted)
# ------------------------------------------------------------------------------------------------------------------------------
BAND = "band width (-w) outside 0 .. 65535: beyond the 16-bit band field of the region keys"
CELLS = "match score x read length beyond the 13-bit DP cells of the extension kernel"
TABLE = "match score above 31 or mismatch penalty above 32: beyond the 6-bit score table of the extension kernel"
GAPS = "gap penalties outside the range of the CIGAR kernels: need open >= 0, extend >= 1, open + 32769 x extend < 2^27"
SEQ311 = np.concatenate([SEQ[:100], np.zeros(211, np.uint8), SEQ[100:]])


def chain_cases(lib, b):
    need = "ssg_dbg_chain: need n_reads >= 0, 1 <= l_pac < 2^33, n_ctg >= 1"
    P = "ssg_dbg_chain: "
    sd, iv = b["seeds"], b["intv"]
    qseed, rseed = "need 0 <= qbeg, 1 <= len, qbeg + len <= read_len: seed ", "need 0 <= rbeg, rbeg + len <= 2 l_pac: seed "
    ivl = "need 0 <= start < end <= read_len: interval "
    return [(dict(), None), (dict(n_reads=0), None), (dict(n_reads=-1), need), (dict(l_pac=0), need), (dict(l_pac=1 << 33), need), (dict(n_ctg=0), need), (dict(n_reads=0, n_ctg=0), need),
            (dict(seed_off=i64(1, 2, 3)), P + "offsets start at 0: read 0"), (dict(intv_off=i64(1, 2, 3)), P + "offsets start at 0: read 0"),
            (dict(seed_off=i64(0, 2, 1)), P + "offsets must not decrease: read 1"), (dict(intv_off=i64(0, 2, 1)), P + "offsets must not decrease: read 1"),
            (dict(seed_off=i64(0, 1 << 24, (1 << 24) + 1)), P + "more than 2^24 seeds or intervals: read 0"),
            (dict(intv_off=i64(0, 2, 2 + (1 << 24))), P + "more than 2^24 seeds or intervals: read 1"),
            (dict(read_len=np.array([0, 80], np.int32)), P + "need 1 <= read_len <= 310: read 0"), (dict(read_len=np.array([100, 311], np.int32)), P + "need 1 <= read_len <= 310: read 1"),
            (dict(seeds=ch(sd, "qbeg", -1)), P + qseed + "0"), (dict(seeds=ch(sd, "len", 0, 2)), P + qseed + "2"), (dict(seeds=ch(sd, "qbeg", 81)), P + qseed + "0"),
            (dict(seeds=ch(sd, "rbeg", -1)), P + rseed + "0"), (dict(seeds=ch(sd, "rbeg", 2 * L_PAC - 19, 1)), P + rseed + "1"),
            (dict(rids=np.array([0, 0, 2], np.int32)), P + "rid beyond the contigs: seed 2"),
            (dict(intv=ch(iv, "info", 30 << 32 | 30)), P + ivl + "0"), (dict(intv=ch(iv, "info", 5 << 32 | 81, 2)), P + ivl + "2"),
            (dict(intv=iv[[1, 0, 2]].copy()), P + "intervals must be sorted by start: interval 1"),
            # two at once: the first in the entry's order wins
            (dict(seed_off=i64(1, 2, 3), read_len=np.array([0, 80], np.int32)), P + "offsets start at 0: read 0"),
            (dict(seed_off=i64(0, 2, 1), read_len=np.array([0, 80], np.int32)), P + "need 1 <= read_len <= 310: read 0"),
            (dict(seeds=ch(ch(sd, "qbeg", -1), "rbeg", -1)), P + qseed + "0"), (dict(seeds=ch(sd, "rbeg", -1), rids=np.array([5, 0, 1], np.int32)), P + rseed + "0"),
            (dict(seeds=ch(sd, "len", 0, 1), intv=ch(iv, "info", 30 << 32 | 30)), P + qseed + "1"),
            (dict(seeds=ch(sd, "len", 0, 2), intv=ch(iv, "info", 30 << 32 | 30)), P + ivl + "0"),
            (dict(intv=ch(iv, "info", 5 << 32 | 200, 1)), P + ivl + "1")]


def regions_cases(lib, b):
    need = "ssg_dbg_regions: need n_reads >= 0, 1 <= l_pac < 2^33, n_ctg >= 1"
    tile = "ssg_dbg_regions: the contigs must tile [0, l_pac) in order"
    P = "ssg_dbg_regions: "
    sd, cn, cs = b["seeds"], b["chains"], b["cs"]
    qseed, rseed = "need 0 <= qbeg, 1 <= len, qbeg + len <= read length: seed ", "need 0 <= rbeg, rbeg + len <= 2 l_pac: seed "
    inside = "every seed of a chain must lie inside the contig and strand of its first seed: chain 0"
    c32 = lambda *v: np.array(v, np.int32)
    return [(dict(), None), (dict(n_reads=0), None), (dict(n_reads=-1), need), (dict(l_pac=0), need), (dict(l_pac=1 << 33), need), (dict(ctg_off=i64(), ctg_len=c32()), need),
            (dict(ctg_len=c32(L0, L1 - 1)), tile), (dict(ctg_len=c32(L0, L1 + 1)), tile), (dict(ctg_off=i64(0, L0 - 1)), tile), (dict(ctg_len=c32(0, L1)), tile), (dict(ctg_off=i64(1, L0)), tile),
            (dict(off=i64(1, 100, 180)), P + "offsets start at 0: read 0"), (dict(seed_off=i64(1, 2, 3)), P + "offsets start at 0: read 0"), (dict(chain_off=i64(1, 1, 2)), P + "offsets start at 0: read 0"),
            (dict(off=i64(0, 100, 90)), P + "offsets must not decrease: read 1"), (dict(seed_off=i64(0, 2, 1)), P + "offsets must not decrease: read 1"),
            (dict(chain_off=i64(0, 1, 0)), P + "offsets must not decrease: read 1"),
            (dict(off=i64(0, 0, 80)), P + "need 1 <= read length <= 310: read 0"), (dict(seq=SEQ311, off=i64(0, 311, 391)), P + "need 1 <= read length <= 310: read 0"),
            (dict(seed_off=i64(0, 1 << 24, (1 << 24) + 1)), P + "more than 2^24 seeds: read 0"), (dict(chain_off=i64(0, 3, 4)), P + "more chains than seeds: read 0"),
            (dict(seq=ch(SEQ, None, 5, 150)), P + "read codes are 0 .. 4: read 1"),
            (dict(seeds=ch(sd, "qbeg", -1)), P + qseed + "0"), (dict(seeds=ch(sd, "len", 0, 2)), P + qseed + "2"), (dict(seeds=ch(sd, "qbeg", 81, 1)), P + qseed + "1"),
            (dict(seeds=ch(sd, "rbeg", -1)), P + rseed + "0"), (dict(seeds=ch(sd, "rbeg", 2 * L_PAC - 19, 1)), P + rseed + "1"),
            (dict(chains=ch(cn, "n", 0)), P + "a chain has at least 1 seed: chain 0"),
            (dict(chains=ch(cn, "first_seed", 1)), P + "first_seed must run on from the chain before: chain 0"),
            (dict(chains=ch(cn, "first_seed", 3, 1)), P + "first_seed must run on from the chain before: chain 1"),
            (dict(cs=ch(cs, None, 2)), P + "a seed index outside the read's seeds: chain 0"), (dict(cs=ch(cs, None, -1, 2)), P + "a seed index outside the read's seeds: chain 1"),
            (dict(cs=ch(cs, None, 0, 1)), P + "a seed in two chains: chain 0"),
            (dict(chains=ch(cn, "rid", 1)), P + "rid must be the contig of the chain's first seed: chain 0"),
            (dict(chains=ch(cn, "rid", 0, 1)), P + "rid must be the contig of the chain's first seed: chain 1"),
            (dict(seeds=ch(sd, "rbeg", L0 - 10, 1)), P + inside), (dict(seeds=ch(sd, "rbeg", L0 + 500, 1)), P + inside), (dict(seeds=ch(sd, "rbeg", L_PAC - 10, 1)), P + inside),
            (dict(seeds=ch(sd, "rbeg", 2 * L_PAC - 1100, 1)), P + inside),
            (dict(opt=opt_with(lib, e_del=0)), P + "gap extension penalties must be positive"), (dict(opt=opt_with(lib, e_ins=0)), P + "gap extension penalties must be positive"),
            (dict(opt=opt_with(lib, a=32)), TABLE), (dict(opt=opt_with(lib, b=33)), TABLE), (dict(opt=opt_with(lib, a=41)), CELLS),
            (dict(opt=opt_with(lib, w=65536)), BAND), (dict(opt=opt_with(lib, w=-1)), BAND),
            # two at once: the contigs before the empty call, the lists in reading order, the lists before the scoring limits, the entry's limits before the stage's
            (dict(n_reads=0, ctg_len=c32(L0, L1 - 1)), tile), (dict(l_pac=0, ctg_len=c32(L0, L1 - 1)), need), (dict(n_reads=0, opt=opt_with(lib, a=32)), None),
            (dict(off=i64(1, 100, 180), ctg_len=c32(L0, L1 - 1)), tile), (dict(off=i64(0, 100, 90), seeds=ch(sd, "qbeg", -1)), P + qseed + "0"),
            (dict(off=i64(0, 0, 80), seed_off=i64(0, 1 << 24, (1 << 24) + 1)), P + "need 1 <= read length <= 310: read 0"),
            (dict(seq=ch(SEQ, None, 5, 50), seeds=ch(sd, "qbeg", -1)), P + "read codes are 0 .. 4: read 0"), (dict(seq=ch(SEQ, None, 5, 150), seeds=ch(sd, "qbeg", -1)), P + qseed + "0"),
            (dict(seeds=ch(sd, "rbeg", -1, 2), chains=ch(cn, "n", 0)), P + "a chain has at least 1 seed: chain 0"),
            (dict(seeds=ch(sd, "rbeg", -1, 1), chains=ch(cn, "n", 0)), P + rseed + "1"),
            (dict(chains=ch(ch(cn, "n", 0), "first_seed", 1)), P + "a chain has at least 1 seed: chain 0"), (dict(chains=ch(cn, "rid", 1), seeds=ch(sd, "rbeg", L0 - 10, 1)), P + "rid must be the contig of the chain's first seed: chain 0"),
            (dict(seeds=ch(sd, "qbeg", -1), opt=opt_with(lib, a=32)), P + qseed + "0"), (dict(opt=opt_with(lib, a=32, e_del=0)), TABLE), (dict(opt=opt_with(lib, a=41, b=33)), CELLS),
            (dict(opt=opt_with(lib, e_del=0, w=65536)), P + "gap extension penalties must be positive"), (dict(opt=opt_with(lib, a=32, w=65536)), TABLE)]


def reg2aln_cases(lib, b):
    need = "ssg_dbg_reg2aln: need n_reads, n_regs >= 0, 0 <= n_req < 2^31, 1 <= l_pac < 2^33, n_ctg >= 1"
    tile = "ssg_dbg_reg2aln: the contigs must tile [0, l_pac) in order"
    P = "ssg_dbg_reg2aln: "
    rg, rq = b["regs"], b["req"]
    span, cross = "need 0 <= rb < re <= 2 l_pac: region ", "a region must not cross the forward / reverse boundary l_pac: region "
    query, both = "need 0 <= qb < qe <= read length: region ", "need 0 <= qb < qe <= read length for the request's region and read: request "
    c32 = lambda *v: np.array(v, np.int32)
    return [(dict(), None), (dict(n_req=0), None), (dict(n_reads=-1), need), (dict(n_regs=-1), need), (dict(n_req=-1), need), (dict(n_req=1 << 31), need), (dict(l_pac=0), need),
            (dict(l_pac=1 << 33), need), (dict(ctg_off=i64(), ctg_len=c32()), need), (dict(ctg_len=c32(L0, L1 - 1)), tile), (dict(ctg_off=i64(0, L0 + 1)), tile),
            (dict(n_reads=0), P + "requests need reads: request 0"), (dict(off=i64(1, 100, 180)), P + "offsets start at 0: read 0"), (dict(off=i64(0, 100, 90)), P + "offsets must not decrease: read 1"),
            (dict(off=i64(0, 0, 80)), P + "need 1 <= read length <= 310: read 0"), (dict(seq=SEQ311, off=i64(0, 311, 391)), P + "need 1 <= read length <= 310: read 0"),
            (dict(seq=ch(SEQ, None, 5, 150)), P + "read codes are 0 .. 4: read 1"),
            (dict(regs=ch(rg, "rb", -1)), P + span + "0"), (dict(regs=ch(rg, "rb", 1100)), P + span + "0"), (dict(regs=ch(ch(rg, "rb", 2 * L_PAC - 50, 1), "re", 2 * L_PAC + 1, 1)), P + span + "1"),
            (dict(regs=ch(ch(rg, "rb", L_PAC - 40), "re", L_PAC + 42)), P + cross + "0"), (dict(regs=ch(rg, "re", 1000 + 32769)), P + "need re - rb <= 32768: region 0"),
            (dict(regs=ch(rg, "qb", -1)), P + query + "0"), (dict(regs=ch(rg, "qb", 80, 1)), P + query + "1"), (dict(regs=ch(rg, "qe", 311)), P + query + "0"),
            (dict(req=ch(rq, "read", 2)), P + "read index out of range: request 0"), (dict(req=ch(rq, "read", -1, 1)), P + "read index out of range: request 1"),
            (dict(req=ch(rq, "reg", 2)), P + "region index out of range: request 0"), (dict(req=ch(rq, "kind", 2, 1)), P + "kind is SSG_REQ_MAIN or SSG_REQ_XA: request 1"),
            (dict(regs=ch(rg, "qe", 101)), P + both + "0"), (dict(req=ch(rq, "read", 1)), P + both + "0"), (dict(req=ch(rq, "reg", -1)), None),
            (dict(opt=opt_with(lib, w=65536)), BAND), (dict(opt=opt_with(lib, w=-1)), BAND), (dict(opt=opt_with(lib, a=32)), TABLE), (dict(opt=opt_with(lib, b=33)), TABLE),
            (dict(opt=opt_with(lib, a=41)), CELLS), (dict(opt=opt_with(lib, e_del=0)), GAPS), (dict(opt=opt_with(lib, o_ins=-1)), GAPS), (dict(opt=opt_with(lib, o_del=1 << 27)), GAPS),
            (dict(opt=opt_with(lib, e_ins=4096)), GAPS),
            # two at once: the contigs before the empty call, the empty call before its lists, reads before regions before requests, the lists before the limits, band / scores / gaps
            (dict(n_req=0, ctg_len=c32(L0, L1 - 1)), tile), (dict(n_req=0, off=i64(1, 100, 90)), None), (dict(n_req=0, opt=opt_with(lib, w=-1)), None),
            (dict(n_reads=0, off=i64(1, 100, 180)), P + "requests need reads: request 0"), (dict(off=i64(0, 100, 90), regs=ch(rg, "rb", -1)), P + "offsets must not decrease: read 1"),
            (dict(seq=ch(SEQ, None, 5, 3), off=i64(0, 100, 90)), P + "read codes are 0 .. 4: read 0"),
            (dict(regs=ch(rg, "rb", -1, 1), req=ch(rq, "read", 2)), P + span + "1"), (dict(regs=ch(ch(rg, "rb", L_PAC - 40), "re", L_PAC + 40000)), P + cross + "0"),
            (dict(regs=ch(ch(rg, "re", 1000 + 32769), "qb", -1)), P + "need re - rb <= 32768: region 0"),
            (dict(req=ch(ch(rq, "read", 2), "kind", 2)), P + "read index out of range: request 0"), (dict(req=ch(ch(rq, "reg", 2), "kind", 2)), P + "region index out of range: request 0"),
            (dict(req=ch(rq, "kind", 2), regs=ch(rg, "qe", 101)), P + "kind is SSG_REQ_MAIN or SSG_REQ_XA: request 0"),
            (dict(req=ch(rq, "kind", 2), opt=opt_with(lib, w=-1)), P + "kind is SSG_REQ_MAIN or SSG_REQ_XA: request 0"),
            (dict(opt=opt_with(lib, w=65536, a=32)), BAND), (dict(opt=opt_with(lib, a=32, e_del=0)), TABLE), (dict(opt=opt_with(lib, a=41, e_del=0)), CELLS)]


def regs_cases(b, L, n_ctg):
    """dbg_check_regs, the validator the three pairing entries share: (change, text behind the entry's name)"""
    rg = b["regs"]
    far = np.minimum(np.arange(65539, dtype=np.int64) * 4096, (1 << 28) + 4096)      # 4096 regions a read: read 65536 is the first to end beyond 2^28
    return [(dict(n_pairs=-1), "n_pairs out of range -1"), (dict(n_pairs=(1 << 24) + 1), "n_pairs out of range 16777217"), (dict(reg_off=i64(1, 1, 2)), "reg_off[0] != 0 0"),
            (dict(reg_off=i64(0, 2, 1)), "reg_off not monotone, or more than 4096 regions in a read: read 1"),
            (dict(reg_off=i64(0, 4097, 4098)), "reg_off not monotone, or more than 4096 regions in a read: read 0"),
            (dict(n_pairs=32769, reg_off=far), "too many regions in all: read 65536"),
            (dict(regs=ch(rg, "rid", n_ctg)), "rid out of range: region 0"), (dict(regs=ch(rg, "rid", -1, 1)), "rid out of range: region 1"),
            (dict(regs=ch(rg, "qe", 311)), "need 0 <= qb < qe <= 310: region 0"), (dict(regs=ch(rg, "qe", 0, 1)), "need 0 <= qb < qe <= 310: region 1"),
            (dict(regs=ch(rg, "qb", -1)), "need 0 <= qb < qe <= 310: region 0"),
            (dict(regs=ch(rg, "rb", -5)), "need 0 <= rb < re <= 2 l_pac: region 0"), (dict(regs=ch(rg, "re", 2 * L + 1, 1)), "need 0 <= rb < re <= 2 l_pac: region 1"),
            (dict(regs=ch(rg, "score", -1)), "score / csub out of range: region 0"), (dict(regs=ch(rg, "csub", (1 << 20) + 1, 1)), "score / csub out of range: region 1"),
            (dict(regs=ch(rg, "frac_rep", 1.5)), "frac_rep outside [0, 1]: region 0"), (dict(regs=ch(rg, "frac_rep", np.nan, 1)), "frac_rep outside [0, 1]: region 1"),
            # two at once
            (dict(n_pairs=-1, reg_off=i64(1, 1, 2)), "n_pairs out of range -1"), (dict(reg_off=i64(1, 0, 2)), "reg_off[0] != 0 0"),
            (dict(reg_off=i64(0, 2, 1), regs=ch(rg, "rid", -1)), "reg_off not monotone, or more than 4096 regions in a read: read 1"),
            (dict(regs=ch(ch(rg, "rid", -1), "qe", 0)), "rid out of range: region 0"), (dict(regs=ch(ch(rg, "qe", 0), "rb", -5)), "need 0 <= qb < qe <= 310: region 0"),
            (dict(regs=ch(ch(rg, "rb", -5), "score", -1)), "need 0 <= rb < re <= 2 l_pac: region 0"), (dict(regs=ch(ch(rg, "score", -1), "frac_rep", 2.0)), "score / csub out of range: region 0"),
            (dict(regs=ch(ch(rg, "frac_rep", 2.0, 1), "score", -1, 1)), "score / csub out of range: region 1"), (dict(regs=ch(ch(rg, "frac_rep", 2.0), "rid", -1, 1)), "frac_rep outside [0, 1]: region 0")]


def pe(pes, **kw):
    p = pes.copy()
    for k, v in kw.items():
        p[k][1] = v
    return p


def pestat_cases(lib, b):
    _, L, n_ctg = example_index(lib)
    P = "ssg_dbg_pestat: "
    c32 = lambda *v: np.array(v, np.int32)
    return [(dict(), None)] + [(kw, P + t) for kw, t in regs_cases(b, L, n_ctg)] + [
        (dict(n_batches=0), P + "1 <= n_batches <= 64"), (dict(n_batches=65), P + "1 <= n_batches <= 64"), (dict(pair_batch=c32(1)), P + "pair_batch out of range"),
        (dict(pair_batch=c32(-1)), P + "pair_batch out of range"), (dict(n_batches=2, pair_batch=c32(1)), None),
        (dict(n_batches=0, regs=ch(b["regs"], "rid", -1)), P + "rid out of range: region 0"), (dict(n_batches=0, pair_batch=c32(-1)), P + "1 <= n_batches <= 64")]


def pair_final_cases(lib, b):
    _, L, n_ctg = example_index(lib)
    P = "ssg_dbg_pair_final: "
    model = P + "an orientation that has not failed needs std > 0 and 0 <= low <= high"
    return [(dict(), None), (dict(n_pairs=0, reg_off=i64(0)), None)] + [(kw, P + t) for kw, t in regs_cases(b, L, n_ctg)] + [
        (dict(pes=pe(b["pes"], std=0.0)), model), (dict(pes=pe(b["pes"], std=np.nan)), model), (dict(pes=pe(b["pes"], low=-1)), model), (dict(pes=pe(b["pes"], low=701)), model),
        (dict(pes=pe(b["pes"], std=0.0, failed=1)), None),
        (dict(pes=pe(b["pes"], std=0.0), regs=ch(b["regs"], "score", -1)), P + "score / csub out of range: region 0"), (dict(pes=pe(b["pes"], std=0.0), n_pairs=0, reg_off=i64(0)), model)]


def matesw_cases(lib, b):
    _, L, n_ctg = example_index(lib)
    P = "ssg_dbg_matesw: "
    model, offs = P + "an orientation that has not failed needs 0 <= low <= high", P + "read_off must start at 0 and increase"
    long_read = "reads longer than 310 bases are outside this build's scope"
    seq, rg = b["seq"], b["regs"]
    seq411 = np.concatenate([seq, np.zeros(211, np.uint8)])
    return [(dict(), None), (dict(n_pairs=0, reg_off=i64(0)), None)] + [(kw, P + t) for kw, t in regs_cases(b, L, n_ctg)] + [
        (dict(pes=pe(b["pes"], low=-1)), model), (dict(pes=pe(b["pes"], low=701)), model), (dict(pes=pe(b["pes"], low=-1, failed=1)), None),
        (dict(read_off=i64(1, 100, 200)), offs), (dict(read_off=i64(0, 100, 100)), offs), (dict(read_off=i64(0, 100, 90)), offs),
        (dict(seq=seq411, read_off=i64(0, 100, 411)), long_read), (dict(seq=ch(seq, None, 5, 150)), P + "bases are codes 0 .. 4"),
        (dict(regs=ch(rg, "qe", 101)), P + "a region ends beyond its read"), (dict(read_off=i64(0, 120, 200)), P + "a region ends beyond its read"),
        (dict(pes=pe(b["pes"], low=-1), regs=ch(rg, "score", -1)), P + "score / csub out of range: region 0"), (dict(pes=pe(b["pes"], low=-1), read_off=i64(1, 100, 200)), model),
        (dict(pes=pe(b["pes"], low=-1), n_pairs=0, reg_off=i64(0)), model), (dict(n_pairs=0, reg_off=i64(0), read_off=i64(1)), None),
        (dict(read_off=i64(0, 100, 100), seq=ch(seq, None, 5)), offs), (dict(seq=ch(seq411, None, 5), read_off=i64(0, 100, 411)), long_read),
        (dict(seq=ch(seq, None, 5, 150), regs=ch(rg, "qe", 101)), P + "bases are codes 0 .. 4")]


def base_sbl_records(lib):
    """one pair: read 1 with a main, an XA and a second main request, read 2 with one main request"""
    req, alns = np.zeros(4, capi.ALNREQ_DT), np.zeros(4, capi.ALN_DT)
    req["kind"] = [0, 1, 0, 0]
    alns["rid"], alns["pos"], alns["flag"], alns["n_cigar"] = [0, 1, 1, 0], [100, 5, 700, 400], [0x40, 0, 0x840, 0x80], 1
    alns["cigar"][:, 0] = 100 << 4
    return dict(req_off=i64(0, 3, 4), req=req, alns=alns, sbl=capi.sbl_opt_init(lib))


def call_sbl_records(lib, a):
    rc, _ = capi.dbg_sbl_records(lib, a["req_off"], a["req"], a["alns"], a["sbl"])
    return answer(lib, rc)


def sbl_records_cases(lib, b):
    P = "ssg_dbg_sbl_records: "
    split = "samblaster: --maxSplitCount above 16 is not supported"
    rq, al = b["req"], b["alns"]
    return [(dict(), None), (dict(req_off=i64(0), req=rq[:0], alns=al[:0]), None), (dict(sbl=capi.sbl_opt_init(lib, max_split_count=16)), None),
            (dict(sbl=capi.sbl_opt_init(lib, max_split_count=17)), split), (dict(sbl=capi.sbl_opt_init(lib, max_split_count=17), req_off=i64(1, 3, 4)), split),
            (dict(req_off=i64(1, 3, 4)), P + "offsets start at 0: read 0"), (dict(req_off=i64(0, 4, 3)), P + "offsets must not decrease: read 1"),
            (dict(req_off=i64(0, 4, 4)), P + "a read without a main request: read 1"), (dict(req=ch(rq, "kind", 1, 3)), P + "a read without a main request: read 1"),
            (dict(req=ch(rq, "kind", 1, 0)), P + "the first request of a read is a main one (its mate's lines print against it): read 0"),
            (dict(req=ch(rq, "kind", 2, 1)), P + "kind is SSG_REQ_MAIN or SSG_REQ_XA: request 1"), (dict(req=ch(rq, "kind", -1, 2)), P + "kind is SSG_REQ_MAIN or SSG_REQ_XA: request 2"),
            (dict(alns=ch(al, "n_cigar", 65, 2)), P + "need 0 <= n_cigar <= 64: record 2"), (dict(alns=ch(al, "n_cigar", -1, 1)), P + "need 0 <= n_cigar <= 64: record 1"),
            (dict(alns=ch(al, "n_cigar", 64, 3)), None), (dict(alns=ch(al, "n_cigar", 0, 0)), None),
            (dict(alns=ch(al, "n_cigar", 65, 3), req_off=i64(0, 3, 2)), P + "offsets must not decrease: read 1"),
            (dict(alns=ch(al, "n_cigar", 65, 3), req=ch(rq, "kind", 1, 0)), P + "the first request of a read is a main one (its mate's lines print against it): read 0")]


ENTRIES = dict(sbl_records=(base_sbl_records, call_sbl_records, sbl_records_cases), chain=(lambda lib: base_chain(), call_chain, chain_cases), regions=(lambda lib: base_regions(), call_regions, regions_cases),
               reg2aln=(lambda lib: base_reg2aln(), call_reg2aln, reg2aln_cases), pestat=(base_pair, call_pestat, pestat_cases),
               pair_final=(base_pair, call_pair_final, pair_final_cases), matesw=(base_pair, call_matesw, matesw_cases))


def check_entry(lib, entry, who):
    base, call, cases = ENTRIES[entry]
    b = base(lib)
    table = cases(lib, b)
    assert table[0] == (dict(), None), "the first case is the valid call"
    for k, (kw, text) in enumerate(table):
        a = dict(b, opt=lib.opt_init())
        a.update(kw)
        got = call(lib, a)
        print("%s case %d %s -> %r" % (entry, k, sorted(kw), got))
        assert got == ((0, "") if text is None else (EINVAL, text)), "%s, ssg_dbg_%s, case %d (%s)" % (who, entry, k, ", ".join(sorted(kw)))


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_emu_refusals(entry, emu_lib):
    check_entry(emu_lib, entry, "the emulation build")


@pytest.mark.gpu
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_gpu_refusals(entry, gpu_lib):
    check_entry(gpu_lib, entry, "the HIP build")
