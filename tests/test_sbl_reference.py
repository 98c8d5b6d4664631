"""Duplicate, discordant and splitter marking (k_sbl.h, k_misc.h and their host side) held to
tests/sbl_reference.py: a reference written from the statement of semantics, with no hash and no packing, on inputs constructed to sit
on the seams of the stage -- the 5' key, the block rules, every threshold of the splitter test, the sort's size classes, equal-hash
runs and the persistent table's slot rule, wrap, growth and contention.

Every constructed case first asserts ON THE REFERENCE ALONE that its seam was reached; then the emulation build, the HIP build and the
oracle's executable are each held to the reference, field for field, with integer equality.  Through: ssg_sbl_markdup,
ssg_sbl_markdup_stream, ssg_sbl_process, the two halves (ssg_sbl_ends -> ssg_sbl_markdup_stream -> ssg_sbl_classify),
ssg_markdup_sig_dev and, from records, the stage test entry ssg_dbg_sbl_records (what ssg_hotpath_dev_ex runs after alignment).
On the MI355X the checks that need device buffers of the caller (ssg_markdup_sig_dev, the hot path of the simulated leg) run in a process
of their own, tests/sbl_check.py, because torch must initialise its HIP runtime before libssgpu is loaded, as in bench.py.

The inputs with a chosen signature hash are built HERE (the mixing function is a bijection, so any hash can be reached from valid ends):
that construction restates the kernel's packing on purpose and is no part of the reference; the verdicts expected of those inputs come
from the reference, which only sees (contig, strand, coordinate).

Two cases are NOT verdicts of the reference (it raises there) and pin the project's choice between the oracle and the builds only:
the pair whose primaries disagree on 0x2 (read 1's flag decides) and pieces with equal query starts whose order changes the marks
(block order decides).
"""
import functools
import os
import re

import numpy as np
import pytest

import common
import sbl_reference as R
from speedseq_amd import capi

M64 = (1 << 64) - 1
SEEN = {}                                           # what each group reached, for profiles/sbl_reference_counts.json (SBL_REFERENCE_COUNTS=path)

# rocPRIM's radix_sort_pairs (rocprim/device/device_radix_sort.hpp) sorts up to block_size * items_per_thread = 256 * 4 items in one block,
# up to radix_sort_config<>::merge_sort_limit = 1024 * 1024 items by merge sort, and only above that by onesweep radix passes
ROCPRIM_SINGLE_SORT_ITEMS = 256 * 4
ROCPRIM_MERGE_SORT_LIMIT = 1024 * 1024
LAUNCH_BLOCK = 256
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, ROCPRIM_SINGLE_SORT_ITEMS - 1, ROCPRIM_SINGLE_SORT_ITEMS, ROCPRIM_SINGLE_SORT_ITEMS + 1, 4097, 70001,
         ROCPRIM_MERGE_SORT_LIMIT + 1]


# ---- lines, blocks and their arrays -----------------------------------------------------------------------------------------------
def end(contig, pos, rev, cigar, mapped=True, mapq=30):
    return dict(contig=contig, pos=pos, rev=rev, cigar=cigar, mapped=mapped, mapq=mapq)


def pair(e1, e2, proper=None, extra=()):
    """the two primary lines of a pair with the FLAG bits a paired-end aligner sets (0x1, 0x2, own / mate 0x4 / 0x8 and 0x10 / 0x20, 0x40 / 0x80);
    extra: lines to add, as (read 1 or 2, end, more FLAG bits)"""
    both = e1["mapped"] and e2["mapped"]
    proper = both if proper is None else proper
    out = []
    for me, mate, bit in ((e1, e2, 0x40), (e2, e1, 0x80)):
        f = 0x1 | bit | (0x2 if proper else 0) | (0 if me["mapped"] else 0x4) | (0 if mate["mapped"] else 0x8) | (0x10 if me["rev"] else 0) | (0x20 if mate["rev"] else 0)
        out.append(R.Line(me["contig"], me["pos"], f, me["mapq"], me["cigar"]))
    for which, e, more in extra:
        me, mate = e, (e2 if which == 1 else e1)
        f = 0x1 | (0x40 if which == 1 else 0x80) | (0x2 if proper else 0) | (0 if e["mapped"] else 0x4) | (0 if mate["mapped"] else 0x8) | (0x10 if e["rev"] else 0) | (0x20 if mate["rev"] else 0) | more
        out.append(R.Line(e["contig"], e["pos"], f, e["mapq"], e["cigar"]))
    return out


UNMAPPED = end(-1, 0, False, "*", mapped=False, mapq=0)
sums = functools.lru_cache(maxsize=None)(R.cigar_sums)


def to_arrays(blocks):
    rows, off = [], [0]
    for b in blocks:
        for l in b:
            lead, trail, q, r = sums(l.cigar)
            rows.append((l.contig, l.pos, l.flag, l.mapq, lead, trail, q, r))
        off.append(len(rows))
    return np.array(off, dtype=np.int64), np.array(rows, dtype=capi.SBL_LINE_DT)


def ends_of(blocks):
    """what a caller of ssg_sbl_markdup hands over: the two primaries of every block as they stand, or two unmapped ends for a block without"""
    rows = []
    for b in blocks:
        r1, r2 = R.primaries(b)
        for i in (r1, r2):
            if r1 < 0 or r2 < 0:
                rows.append((-1, 0, 0x4, 0, 0, 0))
            else:
                lead, trail, _, r = sums(b[i].cigar)
                rows.append((b[i].contig, b[i].pos, b[i].flag, lead, trail, r))
    return np.array(rows, dtype=capi.SBL_END_DT)


def self_ends(case, k):
    return case.ends[k] if case.ends else ends_of(case.stream[k])


def ropt(**kw):
    return R.DEFAULTS._replace(**kw)


def lopt(lib, o):
    return capi.sbl_opt_init(lib, **o._asdict())


class Case:
    def __init__(self, name, stream, opt=None, oracle=True, levels="all"):
        self.name, self.stream, self.opt, self.oracle, self.levels = name, stream, opt or ropt(exclude_dups=1, add_mate_tags=1), oracle, levels
        self._ref, self.ends, self.sigs = None, None, None

    def ref(self):
        """the reference over the whole stream, computed once: per chunk (dup, bits, mate)"""
        if self._ref is None:
            ds = R.DupSet()
            self._ref = [R.process(chunk, self.opt, ds) for chunk in self.stream]
        return self._ref

    def tally(self):
        dups = sum(sum(d) for d, _, _ in self.ref())
        bits = [b for _, bb, _ in self.ref() for b in bb]
        return dict(blocks=sum(len(c) for c in self.stream), calls=len(self.stream), duplicates=dups, discordant_lines=sum(1 for b in bits if b & R.DISC),
                    splitter_lines=sum(1 for b in bits if b & R.SPLIT), lines=len(bits))

    def reached(self, first_slots=1 << 20):
        """tally() and what the stream reaches in the duplicate set, by the serial model below: table sizes, the longest probe and the longest run scanned"""
        m = TableModel(first_slots)
        for chunk in self.stream:
            m.call([R.signature(b) for b in chunk])
        return dict(self.tally(), slots_per_call=m.sizes, longest_probe=m.longest_probe, longest_run_scanned=m.longest_run)


# ---- holding a library and the oracle to the reference ------------------------------------------------------------------------------
def to_host(a):
    return a, a.ctypes.data


def hold_lib(lib, case, to_dev=to_host):
    ref = case.ref()
    o = lopt(lib, case.opt)
    st_whole, st_half, st_ends = (capi.sbl_state_new(lib) for _ in range(3))
    all_sigs = []
    try:
        for k, chunk in enumerate(case.stream):
            rdup, rbits, rmate = ref[k]
            rdup = np.array(rdup, dtype=np.uint8)
            where = "%s call %d" % (case.name, k)
            ends = self_ends(case, k)
            # first-seen-wins through the persistent set, from ends the caller made
            assert np.array_equal(capi.sbl_markdup_stream(lib, st_ends, ends), rdup), where
            if len(case.stream) == 1:
                assert np.array_equal(capi.sbl_markdup(lib, ends), rdup), where
            all_sigs += case.sigs[k] if case.sigs else [R.signature(b) for b in chunk]
            if case.levels != "all":
                continue
            rbits, rmate = np.array(rbits, dtype=np.uint8), np.array(rmate, dtype=np.int64)
            off, lines = to_arrays(chunk)
            # the one-call form
            bits, mate = capi.sbl_process(lib, st_whole, o, off, lines)
            assert np.array_equal(bits, rbits), (where, "bits", np.flatnonzero(bits != rbits)[:8])
            assert np.array_equal(mate, rmate), (where, "mate", np.flatnonzero(mate != rmate)[:8])
            # the two halves, each held to the reference (leg 4)
            e2 = capi.sbl_ends(lib, off, lines)
            dup = capi.sbl_markdup_stream(lib, st_half, e2)
            assert np.array_equal(dup, rdup), (where, "halves dup")
            bits, mate = capi.sbl_classify(lib, o, off, lines, dup)
            assert np.array_equal(bits, rbits) and np.array_equal(mate, rmate), (where, "halves")
            c = R.counts(rdup.tolist(), rbits.tolist())
            assert (int(dup.sum()), int(((bits & 2) != 0).sum()), int(((bits & 4) != 0).sum()), len(bits)) == c
    finally:
        for st in (st_whole, st_half, st_ends):
            capi.sbl_state_free(lib, st)
    if to_dev is not None:
        hold_owner_side(lib, all_sigs, to_dev, case.name)


def hold_owner_side(lib, sigs, to_dev, where, seed=3):
    """ssg_markdup_sig_dev: the stream's signatures as opaque triples (numbered, not packed), handed over in a shuffled order with their ordinals"""
    ids = {None: 0}
    k = np.array([ids.setdefault(s, len(ids)) for s in sigs], dtype=np.uint64)
    raw = np.stack([k * np.uint64(2654435761), k, k * np.uint64(7) + np.uint64(1)], axis=1)
    raw[k == 0] = M64
    perm = np.random.default_rng(seed).permutation(len(sigs))
    sig, ordinal = np.ascontiguousarray(raw[perm]), perm.astype(np.int64)
    order = perm.tolist()
    exp = np.array(R.owner_side([sigs[i] for i in order], order), dtype=np.uint8)
    if len(sigs) <= 70001:
        assert np.array_equal(exp[np.argsort(perm)], np.array(R.DupSet().mark(sigs), dtype=np.uint8))  # the two statements of first-seen-wins agree
    run_sig_dev(lib, sig, ordinal, exp, to_dev, where)


def run_sig_dev(lib, sig, ordinal, exp, to_dev, where):
    dup = np.zeros(len(exp), dtype=np.uint8)
    ks, ko, kd = to_dev(sig), to_dev(ordinal), to_dev(dup)
    capi.markdup_sig_dev(lib, len(exp), ks[1], ko[1], kd[1])
    got = kd[0] if isinstance(kd[0], np.ndarray) else kd[0].cpu().numpy()
    assert np.array_equal(got, exp), (where, "owner side", np.flatnonzero(got != exp)[:8])


def hold_oracle(oracle, case):
    """the oracle's executable on SAM text of the same lines: its three streams against the reference's decisions rendered by the shared writer"""
    blocks = [b for chunk in case.stream for b in chunk]
    n_contigs = 1 + max([l.contig for b in blocks for l in b] + [0])
    assert n_contigs < 100
    text, header = R.sam_text(blocks), R.sam_header(n_contigs)
    bits = [x for _, bb, _ in case.ref() for x in bb]
    mate, base = [], 0
    for chunk, (_, bb, mm) in zip(case.stream, case.ref()):
        mate += [m + base if m >= 0 else -1 for m in mm]
        base += len(bb)
    rm, rd, rs = common.sbl_streams_from_bits(text, bits, mate, bool(case.opt.exclude_dups), bool(case.opt.add_mate_tags))
    out = oracle.samblaster(header + text, exclude_dups=bool(case.opt.exclude_dups), add_mate_tags=bool(case.opt.add_mate_tags), max_split=case.opt.max_split_count,
                            min_non_overlap=case.opt.min_non_overlap)
    rec = lambda t: [l for l in t.split("\n") if l and l[0] != "@"]
    om, od, os_ = rec(out), rec(oracle.last_discordants), rec(oracle.last_splitters)
    assert om == rm, (case.name, "main", [i for i, (a, b) in enumerate(zip(om, rm)) if a != b][:5])
    assert od == rd, (case.name, "discordant", len(od), len(rd))
    assert os_ == rs, (case.name, "splitter", len(os_), len(rs))


# ---- leg 1: the reference against itself, blocks worked by hand --------------------------------------------------------------------
def test_reference_worked_by_hand():
    assert R.cigar_sums("10S5H30M2I3D20M4S") == (15, 4, 52, 53)
    assert R.cigar_sums("5H100M") == (5, 0, 100, 100) and R.cigar_sums("*") == (0, 0, 0, 0) and R.cigar_sums("3M2N3=1X") == (0, 0, 7, 9)
    with pytest.raises(ValueError):
        R.cigar_sums("10S")
    f, r = R.Line(2, 1000, 0x63, 30, "10S90M"), R.Line(2, 1200, 0x93, 30, "5S85M10D5M5H")
    assert R.end_key(f) == (2, 0, 990) and R.end_key(r) == (2, 1, 1200 + 100 - 1 + 5)
    assert R.query_span(f) == (10, 99) and R.query_span(r) == (5, 94)             # the reverse line's query start is its trailing clip
    blk = [f, r]
    assert R.primaries(blk) == (0, 1) and R.signature(blk) == ("pair", ((2, 0, 990), (2, 1, 1304))) == R.signature([r._replace(flag=0x53), f._replace(flag=0xa3)])
    assert R.signature([f, r._replace(flag=0x95)]) == ("orphan", (2, 0, 990)) and R.signature([f._replace(flag=0x65), r._replace(flag=0x95)]) is None
    assert R.signature([f]) is None and R.mate_lines([f]) == [-1]
    sec = R.Line(3, 50, 0x163, 0, "100M")
    assert R.primaries([sec, f, r]) == (1, 2) and R.mate_lines([sec, f, r]) == [2, 2, 1]
    assert R.primaries([f, f._replace(pos=5), r]) == (0, 2)                         # two primaries of read 1: the first counts
    assert R.mark_duplicates([blk, [f._replace(pos=1001), r], blk, [f]]) == [0, 0, 1, 0]
    ds = R.DupSet()
    assert ds.mark([R.signature(blk)]) == [0] and ds.mark([R.signature(blk), None, None]) == [1, 0, 0]
    assert R.owner_side(["a", "b", "a", None, None, "b"], [5, 1, 2, 0, 9, 7]) == [1, 0, 0, 0, 0, 1]
    assert R.discordant(blk) is False and R.discordant([f._replace(flag=0x61), r._replace(flag=0x91)]) is True
    assert R.discordant([f._replace(flag=0x69), r._replace(flag=0x95)]) is False
    with pytest.raises(R.Undefined):
        R.discordant([f._replace(flag=0x61), r])
    o = R.DEFAULTS
    a, b = R.Line(0, 1000, 0x41, 30, "50M100S"), R.Line(1, 5000, 0x841, 30, "50H100M")
    m = R.Line(0, 1300, 0x81, 30, "150M")
    assert R.splitter_lines([a, m, b], 0x40, o) == {0, 2} and R.splitter_lines([a, m, b], 0x80, o) == frozenset()
    assert R.classify([a, m, b], 0, o) == ([R.DISC | R.SPLIT, R.DISC, R.SPLIT], [1, 0, 1])
    assert R.classify([a, m, b], 1, o) == ([7, 3, 5], [1, 0, 1]) and R.classify([a, m, b], 1, o._replace(exclude_dups=1)) == ([1, 1, 1], [1, 0, 1])
    b2 = b._replace(contig=0, pos=1050)                                              # same contig and strand, no indel: not a splitter
    assert R.splitter_lines([a, m, b2], 0x40, o) == frozenset()
    assert R.splitter_lines([a, m, b2._replace(pos=1100)], 0x40, o) == {0, 2} and R.splitter_lines([a, m, b2._replace(pos=1099)], 0x40, o) == frozenset()
    with pytest.raises(R.Tie):
        R.splitter_lines([a, a._replace(contig=2, flag=0x841), b], 0x40, o._replace(max_split_count=3))
    with pytest.raises(ValueError):
        R.splitter_lines([a, m, b], 0x40, o._replace(max_split_count=17))
    assert R.sort_key(r) == (2 << 32 | 1200 << 1 | 1) and R.sort_key(R.Line(-1, 0, 0x4d, 0, "*")) == 0xffffffff << 32 and R.sort_key(f) < R.sort_key(r)
    assert R.counts([0, 1], [7, 3, 5, 0]) == (1, 2, 2, 4)


# ---- leg 2: constructed groups ------------------------------------------------------------------------------------------------------
def group_end_keys():
    F = lambda c, p, cig="100M": end(c, p, False, cig)
    V = lambda c, p, cig="100M": end(c, p, True, cig)
    placed = end(0, 1000, False, "*", mapped=False, mapq=0)                          # flagged 0x4, placed at its mate
    blocks = [
        pair(F(0, 1000), V(0, 1200)),                        # 0  A
        pair(F(0, 1010, "10S90M"), V(0, 1210, "90M")),       # 1  POS traded against the leading clip / the reference length: A again
        pair(F(0, 1005, "5H95M"), V(0, 1200, "90M10S")),     # 2  H forward, trailing S reverse: A again
        pair(F(0, 1000), V(0, 1190, "50M10D40M5S5H")),       # 3  a deletion and S+H behind it: A again
        pair(F(0, 1, "50S50M"), V(0, 1200)),                 # 4  coordinate -49
        pair(F(0, 11, "60S40M"), V(0, 1200)),                # 5  -49 again
        pair(V(0, 901), V(0, 1200)),                         # 6  A but for the strand of one end
        pair(F(1, 1000), V(0, 1200)),                        # 7  A but for the contig of one end
        pair(V(0, 1200), F(0, 1000)),                        # 8  A with the mates swapped
        pair(V(0, 1200), F(1, 1000)),                        # 9  7 with the mates swapped
        pair(F(0, 1000), UNMAPPED),                          # 10 an orphan sharing A's forward end: not A
        pair(UNMAPPED, F(0, 1000)),                          # 11 10 with the unmapped mate as read 1
        pair(F(0, 1000), placed),                            # 12 10 with the unmapped mate placed at its mate
        pair(placed, UNMAPPED), pair(UNMAPPED, UNMAPPED), pair(UNMAPPED, UNMAPPED), pair(placed, placed), pair(UNMAPPED, UNMAPPED),   # 13-17 never
        pair(F(0, 1000), V(0, 901)),                         # 18 equal contig and coordinate, other strand
        pair(V(0, 901), F(0, 1000)),                         # 19 18 swapped
        pair(V(0, 1200), UNMAPPED),                          # 20 an orphan on A's reverse end
        pair(UNMAPPED, V(0, 1190, "50M10D40M5S5H")),         # 21 20 again
    ]
    want = [0, 1, 1, 1, 0, 1, 0, 0, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 1]
    sig = [R.signature(b) for b in blocks]
    assert R.mark_duplicates(blocks) == want
    A = sig[0]
    assert A == ("pair", ((0, 0, 1000), (0, 1, 1299))) and sig[1] == sig[2] == sig[3] == sig[8] == A
    assert sig[4] == sig[5] and sig[4][1][0] == (0, 0, -49)                                                  # below 1
    assert sorted(sig[6][1]) == [(0, 1, 1000), (0, 1, 1299)] and sorted(sig[7][1]) == [(0, 1, 1299), (1, 0, 1000)]   # one field apart from A
    assert sig[10] == sig[11] == sig[12] == ("orphan", (0, 0, 1000)) and all(s is None for s in sig[13:18])
    assert sig[18] == sig[19] == ("pair", ((0, 0, 1000), (0, 1, 1000))) and sig[20] == sig[21] == ("orphan", (0, 1, 1299))
    return [Case("end_keys", [blocks], ropt(add_mate_tags=1))]


def group_blocks():
    F = lambda c, p, cig="150M": end(c, p, False, cig)
    V = lambda c, p, cig="150M": end(c, p, True, cig)
    base = pair(F(0, 1000), V(0, 1400))
    single = [R.Line(0, 1000, 0, 30, "150M")]
    sec_first = [R.Line(2, 77, 0x163, 0, "150M")] + pair(F(0, 1000), V(0, 1400))             # a secondary ahead of its primary
    two_prim = pair(F(0, 1000), V(0, 1400))
    two_prim.insert(1, R.Line(0, 3000, 0x63, 30, "150M"))                                   # a second primary of read 1
    two_prim_other = pair(F(0, 3000), V(0, 1400))                                           # what the second one would pair as: seen for the first time below
    supp_only = [R.Line(1, 500, 0x841, 30, "70M80H"), R.Line(1, 900, 0x91, 30, "150M")]       # read 1 has a supplementary line only
    neither = pair(F(0, 1000), V(0, 1400)) + [R.Line(0, 1000, 0x1, 30, "150M")]              # a line of neither read
    split_disc = pair(end(0, 5000, False, "70M80S"), V(3, 800), proper=False, extra=[(1, end(1, 500, False, "70H80M"), 0x800)])
    blocks = [single, base, single, sec_first, two_prim, two_prim_other, supp_only, supp_only, neither, split_disc, split_disc, pair(UNMAPPED, F(0, 1000)) + [sec_first[0]]]
    want = [0, 0, 0, 1, 1, 0, 0, 0, 1, 0, 1, 0]
    assert R.mark_duplicates(blocks) == want
    assert R.primaries(sec_first) == (1, 2) and R.primaries(two_prim) == (0, 2) and R.primaries(supp_only) == (-1, 1) and R.primaries(single) == (-1, -1)
    cases = []
    for ex in (0, 1):
        c = Case("blocks excludeDups=%d" % ex, [blocks], ropt(exclude_dups=ex, add_mate_tags=1))
        dup, bits, mate = c.ref()[0]
        off, _ = to_arrays(blocks)
        per = [bits[off[i]:off[i + 1]] for i in range(len(blocks))]
        assert per[3] == [1, 1, 1] and per[8] == [1, 1, 1] and per[0] == [0] and per[6] == [0, 0]          # 0x400 on every line of a duplicate block
        assert mate[off[3]:off[4]] == [off[3] + 2, off[3] + 2, off[3] + 1] and mate[off[8]:off[9]] == [off[8] + 1, off[8], -1] and mate[off[6]:off[7]] == [-1, -1]
        assert per[9] == [R.DISC | R.SPLIT, R.DISC, R.SPLIT] and per[10] == ([1, 1, 1] if ex else [7, 3, 5])   # the side streams with and without --excludeDups
        cases.append(c)
    return cases


def group_discordant():
    blocks, want = [], []
    for k, (m1, m2) in enumerate(((1, 1), (1, 0), (0, 1), (0, 0))):
        for proper in (False, True):
            e1 = end(0, 1000 + 10 * len(blocks), False, "100M") if m1 else UNMAPPED
            e2 = end(0, 9000 + 10 * len(blocks), True, "100M") if m2 else UNMAPPED
            blocks.append(pair(e1, e2, proper=proper))
            want.append(m1 and m2 and not proper)
    assert [R.discordant(b) for b in blocks] == want and sum(want) == 1 and len(want) == 8
    assert all((b[0].flag & 0x2) == (0x2 if i & 1 else 0) for i, b in enumerate(blocks))
    return [Case("discordant", [blocks], ropt(add_mate_tags=1))]


def piece(contig, pos, rev, qs, qlen, read_len, extra_ref=0):
    """an aligned piece covering read bases qs .. qs+qlen-1 (counted on the read as sequenced); extra_ref adds a deletion"""
    rest = read_len - qs - qlen
    body = "%dM" % qlen if not extra_ref else "%dM%dD%dM" % (qlen // 2, extra_ref, qlen - qlen // 2)
    lead, trail = (rest, qs) if rev else (qs, rest)
    return end(contig, pos, rev, ("%dS" % lead if lead else "") + body + ("%dS" % trail if trail else ""))


def split_block(pieces, k):
    """read 1 = the pieces (the first is the primary, the rest supplementary), read 2 one line far away; k keeps the pairs' signatures apart"""
    return pair(pieces[0], end(5, 100 + 300 * k, True, "200M"), proper=True, extra=[(1, p, 0x800) for p in pieces[1:]])


def group_splitters():
    RL = 200
    o = ropt(add_mate_tags=1)
    m, ub, ind = o.min_non_overlap, o.max_unmapped_bases, o.min_indel_size
    two = []                                                                           # (pieces, marked?) with max_split_count 2
    P = lambda c, pos, rev, qs, qlen, **kw: piece(c, pos, rev, qs, qlen, RL, **kw)
    two.append(([P(0, 1000, False, 0, 200)], False))                                   # one piece
    two.append(([P(0, 1000, False, 0, 100), P(1, 1000, False, 100, 100)], True))       # two pieces, other contig
    two.append(([P(0, 1000, False, 0, 100), end(1, 1000, False, "100S100M", mapped=False)], False))   # one piece unmapped
    # minNonOverlap: the shorter piece minus the overlap at m-1 and m; one piece inside the other
    two.append(([P(0, 1000, False, 0, 60), P(1, 1000, False, 60 - (60 - m), 60)], True))
    two.append(([P(0, 1000, False, 0, 60), P(1, 1000, False, 60 - (60 - m) - 1, 60)], False))
    two.append(([P(0, 1000, False, 0, 150), P(1, 1000, False, 20, 60)], False))
    # same contig and strand, forward: |ins| at minIndelSize - 1, at it, and negative
    for ins, ok in ((ind - 1, False), (ind, True), (-ind, True), (-(ind - 1), False)):
        two.append(([P(0, 1000, False, 0, 50), P(0, 1000 + 50 + ins, False, 50, 50)], ok))
    # a desert that the insertion explains; unexplained bases at maxUnmappedBases and one more
    two.append(([P(0, 1000, False, 0, 50), P(0, 1000 + 130 + 60, False, 130, 50)], True))           # desert 80, ins 60
    two.append(([P(0, 1000, False, 0, 50), P(0, 1000 + 130 - 60, False, 130, 50)], False))          # desert 80, ins -60
    two.append(([P(0, 1000, False, 0, 50), P(0, 1000 + 50 + ub - ind, False, 50 + ub, 50)], True))  # desert ub, ins -ind
    two.append(([P(0, 1000, False, 0, 50), P(0, 1000 + 51 + ub - ind, False, 51 + ub, 50)], False)) # desert ub + 1
    # other contig, other strand: the desert at the limit and one more
    for c, rev in ((1, False), (0, True)):
        two.append(([P(0, 1000, False, 0, 50), P(c, 3000, rev, 50 + ub, 50)], True))
        two.append(([P(0, 1000, False, 0, 50), P(c, 3000, rev, 51 + ub, 50)], False))
    # reverse pieces: the query start is the trailing clip, the reference runs backwards
    for ins, ok in ((ind - 1, False), (ind, True), (-ind, True), (-(ind - 1), False)):
        two.append(([P(0, 5000, True, 0, 50), P(0, 5000 - 50 - ins, True, 50, 50)], ok))
    two.append(([P(0, 5000, True, 0, 50), P(0, 5000 - 130 - 60, True, 130, 50)], True))              # desert 80 explained by ins 60
    two.append(([P(0, 5000, True, 0, 50), P(0, 5000 - 130 + 60, True, 130, 50)], False))
    # the reference length of a reverse piece counts, deletions included: last bases 5056 and pos + 52, so ins = 4954 - pos (46 and 45 without the deletions)
    two.append(([P(0, 5000, True, 0, 50, extra_ref=7), P(0, 4954 - ind, True, 50, 50, extra_ref=3)], True))
    two.append(([P(0, 5000, True, 0, 50, extra_ref=7), P(0, 4954 - ind + 1, True, 50, 50, extra_ref=3)], False))
    two.append(([P(0, 1000, False, 0, 100), P(1, 1000, False, 0, 100)], False))        # equal query starts, two pieces: no order marks them
    blocks = [split_block(p, k) for k, (p, _) in enumerate(two)]
    got = [bool(R.splitter_lines(b, 0x40, o)) for b in blocks]
    want = [ok for _, ok in two]
    assert got == want, [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert sum(want) >= 9 and want.count(False) >= 9
    cases = [Case("splitters max 2", [blocks], o)]
    # piece counts against maxSplitCount: 2, max, max + 1 with max 3; 16 and 17 with max 16
    chain = lambda n, w: [piece(i % 4, 1000 + 100 * i, False, i * w, w, n * w) for i in range(n)]
    o3, o16 = o._replace(max_split_count=3), o._replace(max_split_count=16)
    mid = [piece(0, 1000, False, 0, 50, 150), piece(1, 1000, False, 50, 50, 150), piece(1, 1050, False, 100, 50, 150)]   # the middle piece qualifies with its left neighbour only
    quiet = [piece(0, 1000, False, 0, 40, 300), piece(1, 1000, False, 0, 60, 300), piece(2, 1000, False, 200, 100, 300)]  # equal starts; the third is out of reach of both: no Tie
    b3 = [split_block(chain(2, 50), 0), split_block(chain(3, 50), 1), split_block(chain(4, 50), 2), split_block(mid, 3), split_block(quiet, 4)]
    assert [sorted(R.splitter_lines(b, 0x40, o3)) for b in b3] == [[0, 2], [0, 2, 3], [], [0, 2], []]
    cases.append(Case("splitters max 3", [b3], o3))
    b16 = [split_block(chain(16, 30), 0), split_block(chain(17, 30), 1), split_block(chain(2, 30), 2)]
    assert [len(R.splitter_lines(b, 0x40, o16)) for b in b16] == [16, 0, 2]
    cases.append(Case("splitters max 16", [b16], o16))
    for c in cases:
        assert c.tally()["splitter_lines"] > 0
    return cases


def pinned_cases():
    """where the reference raises: the project's choice, restated here and held between the oracle and the builds only"""
    und = [pair(end(0, 1000, False, "100M"), end(0, 9000, True, "100M"), proper=False), pair(end(0, 2000, False, "100M"), end(0, 9500, True, "100M"), proper=True)]
    und[0][1] = und[0][1]._replace(flag=und[0][1].flag | 0x2)                       # read 1 without 0x2, read 2 with it: discordant
    und[1][1] = und[1][1]._replace(flag=und[1][1].flag & ~0x2)                      # read 1 with 0x2, read 2 without: not
    und[1].reverse()                                                                # ... with read 2 first in the block
    tie = split_block([piece(0, 1000, False, 0, 50, 100), piece(1, 1000, False, 0, 50, 100), piece(2, 1000, False, 50, 50, 100)], 0)
    # read 1 has two pieces that qualify as splitters but no primary among them (both 0x800)
    orphaned = pair(piece(0, 1000, False, 0, 50, 100), end(5, 400, True, "200M"), proper=True, extra=[(1, piece(1, 1000, False, 50, 50, 100), 0x800)])
    orphaned[0] = orphaned[0]._replace(flag=orphaned[0].flag | 0x800)
    assert R.primaries(orphaned) == (-1, 1) and R.splitter_lines(orphaned, 0x40, ropt()) == {0, 2}
    with pytest.raises(R.Undefined):
        R.classify(orphaned, 0, ropt())
    for b in und:
        with pytest.raises(R.Undefined):
            R.discordant(b)
    with pytest.raises(R.Tie):
        R.splitter_lines(tie, 0x40, ropt(max_split_count=3))
    # read 1's 0x2 decides; among equal query starts the block's order stands (the later line is the neighbour of the next piece); a block without two
    # primaries reaches no side stream
    return [("undefined 0x2", [und], ropt(add_mate_tags=1), [[R.DISC, R.DISC, 0, 0]]),
            ("splitters without two primaries", [[orphaned]], ropt(add_mate_tags=1), [[0, 0, 0]]),
            ("tie", [[tie]], ropt(add_mate_tags=1, max_split_count=3), [[0, 0, R.SPLIT, R.SPLIT]])]


def random_pairs(n, seed, dup_third=True, contigs=3, span=1 << 22):
    """n pairs, about a third of them duplicates of an earlier one in another composition (clip traded against POS, mates swapped)"""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 3, size=n)
    src = (rng.random(n) * np.arange(n)).astype(np.int64)
    c1, c2 = rng.integers(0, contigs, size=n), rng.integers(0, contigs, size=n)
    p1, p2 = rng.integers(100, span, size=n), rng.integers(100, span, size=n)
    clip, swap, orphan = rng.integers(0, 30, size=n), rng.integers(0, 2, size=n), rng.integers(0, 25, size=n)
    ends, blocks = [], []
    for i in range(n):
        if dup_third and kind[i] == 0 and i:
            a, b = ends[src[i]]
        else:
            a = (int(c1[i]), 0, int(p1[i])) if orphan[i] != 1 else None
            b = (int(c2[i]), 1, int(p2[i])) if orphan[i] != 2 else None
        ends.append((a, b))
        k = int(clip[i])
        e1 = end(a[0], a[2] + k, False, "%dS%dM" % (k, 100 - k) if k else "100M") if a else UNMAPPED
        e2 = end(b[0], b[2] - 99, True, "%dM%dS" % (100 - k, k) if k else "100M") if b else UNMAPPED      # POS + reference length - 1 + clip = b[2]
        blocks.append(pair(e2, e1) if swap[i] else pair(e1, e2))
    return blocks


def big_ends(n, seed):
    """n pairs of ends as arrays (no lines: past 70001 pairs only the duplicate verdicts are held, the sort being all that changes with the size) and
    their signatures by the reference's rule; a third are copies of an earlier pair with the mates swapped"""
    rng = np.random.default_rng(seed)
    orig = np.flatnonzero((rng.integers(0, 3, size=n) != 0) | (np.arange(n) == 0))
    before = np.searchsorted(orig, np.arange(n), side="right")                       # originals at or before each pair
    src = orig[np.minimum((rng.random(n) * before).astype(np.int64), before - 1)]
    copy = np.ones(n, dtype=bool); copy[orig] = False
    src[~copy] = np.arange(n)[~copy]
    c = rng.integers(0, 24, size=(n, 2))[src]; p = rng.integers(1, 1 << 27, size=(n, 2))[src]
    ends = np.zeros(2 * n, dtype=capi.SBL_END_DT)
    swap = copy & (rng.integers(0, 2, size=n) == 1)
    for e in (0, 1):                                                                 # end 0 forward at p, end 1 reverse with its last base at p
        at = np.where(swap, 1 - e, e) + 2 * np.arange(n)
        ends["seq"][at] = c[:, e]; ends["pos"][at] = p[:, e]; ends["ralen"][at] = 100
        ends["flag"][at] = np.where(swap, (0xa3, 0x53)[e], (0x63, 0x93)[e])
    fwd = list(zip(c[:, 0].tolist(), [0] * n, p[:, 0].tolist()))                     # the end keys, spelled out: (contig, strand, 5' coordinate)
    rev = list(zip(c[:, 1].tolist(), [1] * n, (p[:, 1] + 99).tolist()))
    sigs = [("pair", (a, b) if a <= b else (b, a)) for a, b in zip(fwd, rev)]
    return ends, sigs


@functools.lru_cache(maxsize=None)
def sizes_case(n):
    if n > 70001:
        c = Case("sizes %d" % n, [None], ropt(add_mate_tags=1), oracle=False, levels="dup")
        ends, sigs = big_ends(n, seed=n)
        c.ends, c.sigs, c._ref = [ends], [sigs], [(R.DupSet().mark(sigs), None, None)]
    else:
        c = Case("sizes %d" % n, [random_pairs(n, seed=100 + n % 97)], ropt(add_mate_tags=1))
    d = sum(c.ref()[0][0])
    assert n < 64 or n // 5 < d < n // 2, (n, d)                                     # about a third
    return c


# ---- inputs with a chosen signature hash (the kernel's mixing and packing restated to BUILD inputs; never to judge them) ------------
def mix64(x):
    x ^= x >> 33; x = x * 0xff51afd7ed558ccd & M64; x ^= x >> 33; x = x * 0xc4ceb9fe1a85ec53 & M64; x ^= x >> 33
    return x


INV1, INV2 = pow(0xff51afd7ed558ccd, -1, 1 << 64), pow(0xc4ceb9fe1a85ec53, -1, 1 << 64)


def unmix64(x):
    x ^= x >> 33; x = x * INV2 & M64; x ^= x >> 33; x = x * INV1 & M64; x ^= x >> 33
    return x


def packed_hash(sig, p):
    """the 64-bit hash the kernels give a reference signature (pair p of its call stands in with 2^64 - 1 - p when it has none): the packing restated, for
    TableModel and the counts file only"""
    if sig is None:
        return M64 - p
    if sig[0] == "orphan":
        c, st, q = sig[1]
        return mix64(c ^ mix64(((q + (1 << 31)) << 1 | st) ^ mix64(0)))
    lo, hi = sorted(sig[1], key=lambda k: (k[0], k[2], k[1]))
    return mix64((lo[0] << 32 | hi[0]) ^ mix64(((lo[2] + (1 << 31)) << 1 | lo[1]) ^ mix64((hi[2] + (1 << 31)) << 1 | hi[1])))


class TableModel:
    """A serial model of the persistent duplicate set as DESIGN describes it (open addressing, linear probing, slot value 0 = empty so hash 0 is kept as 1, sized
    for twice the pairs handed over, grown by doubling with every entry put again in slot order), fed with reference signatures.  It judges nothing: it says
    which seam a constructed stream reaches -- table sizes, the longest probe (slots read by a look-up or an insertion) and the longest backward scan of an
    equal-hash run -- for the groups' own assertions and for the counts file.  The kernels insert concurrently, so their probes may differ in length."""

    def __init__(self, first_slots):
        self.first, self.slots, self.n, self.at, self.free, self.sizes, self.longest_probe, self.longest_run, self.wrapped = first_slots, 0, 0, {}, {}, [], 0, 0, 0

    def _find(self, q):
        path = []
        while q in self.free:
            path.append(q); q = self.free[q]
        for x in path:
            self.free[x] = q
        return q

    def _put(self, sig, h):
        mask = self.slots - 1
        q0 = (h or 1) & mask
        q = self._find(q0)
        self.free[q] = (q + 1) & mask
        self.at[sig] = (q, h, ((q - q0) & mask) + 1)
        self.wrapped += q < q0
        self.longest_probe = max(self.longest_probe, ((q - q0) & mask) + 1)

    def call(self, sigs):
        want = self.slots or self.first
        while (self.n + len(sigs)) * 2 > want:
            want *= 2
        if want != self.slots:
            old = sorted(self.at.items(), key=lambda kv: kv[1][0])
            self.slots, self.at, self.free = want, {}, {}
            for sig, (_, h, _) in old:
                self._put(sig, h)
        mask, runs, fresh = self.slots - 1, {}, []
        for p, sig in enumerate(sigs):
            h = packed_hash(sig, p)
            run, found, steps = runs.setdefault(h, []), False, 0
            if sig is not None:
                for t in reversed(run):
                    steps += 1
                    if t == sig:
                        found = True
                        break
                self.longest_run = max(self.longest_run, steps)
                if not found:
                    if sig in self.at:
                        self.longest_probe = max(self.longest_probe, self.at[sig][2])
                    else:
                        q0 = (h or 1) & mask
                        self.longest_probe = max(self.longest_probe, ((self._find(q0) - q0) & mask) + 1)
                        fresh.append((sig, h))
            run.append(sig)
        for sig, h in fresh:
            self._put(sig, h)
        self.n += len(sigs)
        self.sizes.append(self.slots)


def pairs_with_hashes(hashes, rng):
    """for each hash a pair of valid mapped ends (contig ids below 2^31) whose signature hashes to it, all with the SAME coordinates and strands (they differ
    in their contigs only), and the number of draws it took"""
    draws = 0
    while True:
        draws += 1
        (q1, q2), (s1, s2) = (int(x) for x in rng.integers(1000, 1 << 28, size=2)), (int(x) for x in rng.integers(0, 2, size=2))
        k1, k2 = (q1 + (1 << 31)) << 1 | s1, (q2 + (1 << 31)) << 1 | s2
        k0 = [unmix64(h) ^ mix64(k1 ^ mix64(k2)) for h in hashes]
        if any(k >> 32 >= 1 << 31 or k & 0xffffffff >= 1 << 31 or (k >> 32, q1, s1) > (k & 0xffffffff, q2, s2) for k in k0):
            continue
        assert [mix64(k ^ mix64(k1 ^ mix64(k2))) for k in k0] == list(hashes)
        mk = lambda c, q, s: end(c, q - 99, True, "100M") if s else end(c, q, False, "100M")
        return [pair(mk(k >> 32, q1, s1), mk(k & 0xffffffff, q2, s2)) for k in k0], draws


def pair_with_hash(h, rng):
    blocks, draws = pairs_with_hashes([h], rng)
    return blocks[0], draws


def distinct(blocks):
    sig = [R.signature(b) for b in blocks]
    assert None not in sig and len(set(sig)) == len(sig)
    return blocks


def group_equal_hash_runs():
    rng = np.random.default_rng(17)
    H = [int(x) for x in rng.integers(0, 1 << 63, size=3)]
    runs = [distinct([pair_with_hash(h, rng)[0] for _ in range(n)]) for h, n in zip(H, (2, 3, 64))]
    flat = [b for r in runs for b in r]
    distinct(flat)
    first = [flat[i] for i in rng.permutation(len(flat))]
    # call 0: every signature of a run and its repeat, interleaved (A B A' C B' ...); call 1: a run-mate of each hash for the first time, then repeats
    mixed = first + [flat[i] for i in rng.permutation(len(flat))]
    order = np.argsort(np.concatenate([np.arange(len(first)) * 2.0, np.arange(len(first)) * 2.0 + 2.5 + rng.integers(0, 9, size=len(first))]), kind="stable")
    call0 = [mixed[i] for i in order]
    late = distinct([pair_with_hash(h, rng)[0] for h in H for _ in range(2)])
    distinct(flat + late)
    call1 = late[:3] + [flat[0], flat[2], flat[7]] + late[3:] + late[:2]
    d0 = R.mark_duplicates(call0)
    assert sum(d0) == len(flat) and d0[0] == 0 and d0[-1] == 1 and 1 in d0[:len(flat)] and 0 in d0[len(flat) // 2:]   # repeats sit between first sightings
    cases = [Case("equal_hash_runs", [call0, call1], ropt(add_mate_tags=1), oracle=False)]
    assert cases[0].ref()[1][0] == [0, 0, 0, 1, 1, 1, 0, 0, 0, 1, 1]
    # a mapped pair whose hash is the stand-in of an unmapped pair of the same call: 2^64 - 1 - p for pair p
    n = 12
    blocks = [pair(UNMAPPED, UNMAPPED) for _ in range(n)]
    for p_unmapped, at in ((3, 0), (1, 5), (2, 9), (10, 11)):
        blocks[at] = pair_with_hash(M64 - p_unmapped, rng)[0]
    assert all(R.signature(blocks[p]) is None for p in (3, 1, 2, 10))
    blocks += [blocks[0], blocks[5], blocks[11]]
    assert R.mark_duplicates(blocks) == [0] * n + [1, 1, 1]
    cases.append(Case("stand-in hash", [blocks], ropt(add_mate_tags=1), oracle=False))
    reached = cases[0].reached()
    assert reached["longest_run_scanned"] >= 64, reached                            # a scan that passes every other signature of the run of 64 before its match
    assert cases[1].reached()["longest_run_scanned"] >= 1                            # a mapped pair sorted next to the unmapped pair whose stand-in hash it has
    return cases


def raw_equal_hash(lib, to_dev):
    """ssg_markdup_sig_dev with raw signatures that share one hash, and shuffled ordinals"""
    rng = np.random.default_rng(23)
    sig = []
    for h, n in ((int(rng.integers(0, 1 << 63)), 64), (0, 3), (M64, 2)):
        for _ in range(n):
            k1, k2 = (int(x) for x in rng.integers(0, 1 << 62, size=2))
            k0 = unmix64(h) ^ mix64(k1 ^ mix64(k2))
            assert mix64(k0 ^ mix64(k1 ^ mix64(k2))) == h
            sig.append((k0, k1, k2))
    assert len(set(sig)) == len(sig)
    rows = sig * 3 + [(M64, M64, M64)] * 5
    perm = rng.permutation(len(rows))
    rows = [rows[i] for i in perm]
    ordinal = rng.permutation(10 * len(rows))[:len(rows)].astype(np.int64)
    exp = np.array(R.owner_side([None if r == (M64, M64, M64) else r for r in rows], [int(x) for x in ordinal]), dtype=np.uint8)
    assert int(exp.sum()) == 2 * len(sig)
    run_sig_dev(lib, np.array(rows, dtype=np.uint64), ordinal, exp, to_dev, "raw equal-hash signatures")


@functools.lru_cache(maxsize=None)
def table_cases(which):
    """streams for a persistent table that starts at 16 slots (SSG_SBL_TABLE_SLOTS=16).  The host side sizes the table for twice the pairs
    handed over so far, this call's included, so the load factor stays at or below 1/2 and the table is never full."""
    rng = np.random.default_rng(29)
    if which == "slot rule":                                                     # hash 0 is stored as 1: two signatures, one slot value
        X, Y = pair_with_hash(0, rng)[0], pair_with_hash(1, rng)[0]
        distinct([X, Y])
        c = Case("table: hash 0 and hash 1", [[X], [Y, X, Y]], oracle=False)
        assert [d for d, _, _ in c.ref()] == [[0], [0, 1, 1]]
        reached = c.reached(16)
        assert reached["slots_per_call"] == [16, 16] and reached["longest_probe"] == 2, reached     # Y probes past X in slot 1
    elif which == "wrap":                                                        # three signatures at home in the last of 16 slots, looked up in the next call
        S = distinct([pair_with_hash(int(rng.integers(0, 1 << 59)) << 4 | 15, rng)[0] for _ in range(4)])
        c = Case("table: probe wraps", [S[:3], [S[2], S[1], S[0], S[3]]], oracle=False)
        assert [d for d, _, _ in c.ref()] == [[0, 0, 0], [1, 1, 1, 0]]
        m = TableModel(16)
        m.call([R.signature(b) for b in c.stream[0]])
        assert m.sizes == [16] and m.wrapped == 2 and sorted(v[0] for v in m.at.values()) == [0, 1, 15]   # the probe went round the end of the table
        reached = c.reached(16)
        assert reached["slots_per_call"] == [16, 16] and reached["longest_probe"] == 4, reached
    elif which == "growth":                                                      # 8 calls of 3000 pairs; every earlier signature again after each rehash
        fresh = distinct(random_pairs(8 * 375, seed=31, dup_third=False, span=1 << 26))
        stream = []
        for k in range(8):
            pad = [fresh[int(i)] for i in rng.integers(0, 375 * (k + 1), size=3000 - 375 * (k + 1))]
            chunk = fresh[:375 * (k + 1)] + pad
            stream.append([chunk[int(i)] for i in rng.permutation(3000)])
        c = Case("table: growth", stream)
        reached = c.reached(16)
        assert [sum(d) for d, _, _ in c.ref()] == [3000 - 375] * 8 and len(set(reached["slots_per_call"])) >= 4 and reached["slots_per_call"][0] > 16, reached
    else:                                                                        # 4096 new signatures with one home slot in any table of up to 2^20 slots
        low, draws = 0x5a5a5, 0
        S = []
        for _ in range(8192):
            b, d = pair_with_hash(int(rng.integers(0, 1 << 43)) << 20 | low, rng)
            S.append(b); draws += d
        distinct(S)
        c = Case("table: contention", [S[:4096], [S[int(i)] for i in rng.permutation(8192)]], oracle=False)
        assert [sum(d) for d, _, _ in c.ref()] == [0, 4096]
        reached = c.reached(16)
        assert reached["longest_probe"] >= 8192 and all(2 * 4096 * (k + 1) <= n for k, n in enumerate(reached["slots_per_call"])), reached   # load factor <= 1/2
        reached["draws_per_pair"] = round(draws / 8192, 2)
    SEEN["table: " + which] = reached
    return c


# ---- records: through ssg_dbg_sbl_records ----------------------------------------------------------------------------------------
OPS = "MIDSH"


def rec(rid, pos, rev, cigar, flag, mapq=30, main=True):
    ops = tuple((int(n), op) for n, op in re.findall(r"(\d+)([MIDSH])", cigar))
    return R.Rec(main, rid, pos, flag, mapq, 1 if rev else 0, ops)


UNREC = lambda flag: R.Rec(True, -1, -1, flag, 0, 0, ())


def recs_to_arrays(pairs):
    """(req_off, req, alns) as the pairing and record stages leave them: read 1 and read 2 of a pair interleaved, a record per request"""
    off, kinds, rows = [0], [], []
    for p in pairs:
        for read in p:
            for r in read:
                kinds.append(0 if r.main else 1)
                rows.append(r)
            off.append(len(rows))
    req, alns = np.zeros(len(rows), capi.ALNREQ_DT), np.zeros(len(rows), capi.ALN_DT)
    req["kind"] = kinds
    for k, r in enumerate(rows):
        a = alns[k]
        a["pos"], a["rid"], a["flag"], a["mapq"], a["is_rev"], a["n_cigar"] = r.pos, r.rid, r.flag, r.mapq, r.is_rev, len(r.cigar)
        a["cigar"][:len(r.cigar)] = [n << 4 | OPS.index(op) for n, op in r.cigar]
    return np.array(off, np.int64), req, alns


def records_cases():
    A = lambda f=0x42: rec(0, 999, False, "100M", f)
    B = lambda f=0x82: rec(0, 1200, True, "100M", f)
    xa = rec(1, 5, False, "100M", 0, main=False)
    pairs = [
        ([A()], [B()]),                                                                         # 0  a proper pair
        ([UNREC(0x40)], [B(0x80)]),                                                             # 1  read 1 unmapped: placed at its mate, 0x4, 0x10 and 0x20 from the mate
        ([A(0x40)], [UNREC(0x80)]),                                                             # 2  the reverse: 0x8, and 0x20 from the read itself
        ([UNREC(0x40)], [UNREC(0x80)]),                                                         # 3  both unmapped
        ([rec(0, 4999, False, "70M80S", 0x40), rec(1, 499, False, "70H80M", 0x840)], [rec(3, 800, True, "150M", 0x80)]),   # 4 supplementary with hard clips: discordant, splitter
        ([rec(0, 5999, False, "70M80S", 0x42), rec(1, 499, False, "70H80M", 0x10042)], [rec(0, 6300, True, "150M", 0x82)]),  # 5 the internal secondary bit prints as 0x100
        ([A(), xa, rec(2, 700, True, "40H60M", 0x842), xa], [xa._replace(main=True, flag=0x82, rid=0, pos=1200, is_rev=1), xa, xa]),   # 6 XA requests between main ones: 0 again
        ([rec(0, 7000, False, "", 0x42)], [rec(0, 7300, True, "", 0x82)]),                       # 7  n_cigar 0
        ([rec(0, 8004, False, "5S30M5I40M7D20M3S", 0x42)], [rec(0, 8300, True, "2S3H50M4D45M6S1H", 0x82)]),   # 8 I and D, clips at both ends
        ([rec(0, 8009, False, "10S25M5I40M7D20M3H", 0x42)], [rec(0, 8301, True, "49M4D45M7S", 0x82)]),       # 9 8 again, composed differently
        ([B(0x42)], [A(0x82)]),                                                                 # 10 0 with the mates swapped
        ([UNREC(0x40)], [B(0x80)]),                                                             # 11 1 again
    ]
    blocks = [R.record_lines(*p) for p in pairs]
    f = lambda b: [l.flag for l in b]
    assert f(blocks[0]) == [0x63, 0x93] and f(blocks[1]) == [0x75, 0xb9] and f(blocks[2]) == [0x49, 0x85] and f(blocks[3]) == [0x4d, 0x8d]
    assert blocks[1][0][:2] == (0, 1201) and blocks[1][0].cigar == "*" and blocks[3][0][:2] == (-1, 0)
    assert f(blocks[4]) == [0x61, 0x861, 0x91] and f(blocks[5]) == [0x63, 0x163, 0x93] and len(blocks[6]) == 3 and blocks[7][0].cigar == "*"
    assert [R.cigar_sums(l.cigar) for l in blocks[8]] == [(5, 3, 95, 97), (5, 7, 95, 99)]
    c = Case("records", [blocks], ropt(add_mate_tags=1))
    assert c.ref()[0][0] == [0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 1]
    return pairs, c


def hold_records(lib, pairs, case, st=None, dupset=None):
    """ssg_dbg_sbl_records on the records of one call against the reference, output by output; returns what was left out (blocks the reference raises on)"""
    blocks = case.stream[0]
    rdup, rbits, rmate = case.ref()[0]
    req_off, req, alns = recs_to_arrays(pairs)
    rc, o = capi.dbg_sbl_records(lib, req_off, req, alns, lopt(lib, case.opt), st)
    lib._chk(rc)
    off, lines = to_arrays(blocks)
    assert np.array_equal(o["line_off"], off) and len(o["lines"]) == len(lines)
    for fld in capi.SBL_LINE_DT.names:
        assert np.array_equal(o["lines"][fld], lines[fld]), (case.name, fld, np.flatnonzero(o["lines"][fld] != lines[fld])[:8])
    main = np.flatnonzero(req["kind"] == 0)
    assert np.array_equal(o["line_req"], main)                                                 # the request each line prints: the main ones in order
    prim = np.array([[off[b] + i if i >= 0 else -1 for i in R.primaries(blk)] for b, blk in enumerate(blocks)], np.int64).reshape(-1)
    assert np.array_equal(o["prim"], prim)
    sig = [R.signature(b) for b in blocks]
    for b, blk in enumerate(blocks):
        for e in (0, 1):
            got, l = o["ends"][2 * b + e], blk[prim[2 * b + e] - off[b]]
            if R.is_mapped(l):
                lead, trail, _, r = sums(l.cigar)
                assert tuple(int(x) for x in got.tolist()) == (l.contig, l.pos, l.flag, lead, trail, r), (b, e)
            else:
                assert got["seq"] == -1 and got["flag"] & 0x4
    # the signatures without knowing their packing: equal words iff equal signatures, all ones iff none
    words = [tuple(int(x) for x in w) for w in o["sig"]]
    seen = {}
    for w, s_ in zip(words, sig):
        assert (w == (M64, M64, M64)) == (s_ is None)
        if s_ is not None:
            assert seen.setdefault(w, s_) == s_
    assert len({w for w, s_ in zip(words, sig) if s_ is not None}) == len({s_ for s_ in sig if s_ is not None})
    assert o["dup"].tolist() == rdup and o["bits"].tolist() == rbits and o["mate"].tolist() == rmate
    assert tuple(int(x) for x in o["counts"]) == R.counts(rdup, rbits)
    assert [int(k) for k in o["keys"]] == [R.sort_key(l) for b in blocks for l in b]
    return o


def hold_records_group(lib):
    pairs, case = records_cases()
    hold_records(lib, pairs, case)
    SEEN["records"] = dict(cases={case.name: case.tally()})
    o = lopt(lib, ropt(max_split_count=17))                                                    # refused on the host, before any launch
    req_off, req, alns = recs_to_arrays(pairs)
    rc, _ = capi.dbg_sbl_records(lib, req_off, req, alns, o)
    assert rc == -22


# ---- leg 3: simulated pairs through the timed step -----------------------------------------------------------------------------------
def recs_of_result(res):
    """the downloaded records of a call as R.Rec lists per read"""
    pairs, off = [], res.req_off
    for p in range(len(off) // 2):
        reads = []
        for r in (2 * p, 2 * p + 1):
            reads.append([R.Rec(int(res.req["kind"][g]) == 0, int(a["rid"]), int(a["pos"]), int(a["flag"]), int(a["mapq"]), int(a["is_rev"]),
                                tuple((int(c) >> 4, OPS[int(c) & 0xf]) for c in a["cigar"][:int(a["n_cigar"])])) for g, a in ((g, res.alns[g]) for g in range(off[r], off[r + 1]))])
        pairs.append(tuple(reads))
    return pairs


def hold_simulated(lib, n_pairs, per, read_len, to_dev):
    """the step of common.check_hotpath (seed 41, dup_frac 0.1) against the reference: lines from the downloaded records = lines of the printed text; the
    device's dup, bits, mate lines and counts = the reference's.  Blocks on which the reference raises are left out and counted: at most 1 %."""
    kw = dict(ins_mean=800, ins_std=150) if read_len > 200 else {}
    pairs, seqs, seq, off = common.sim_reads(n_pairs, seed=41, read_len=read_len, dup_frac=0.1, **kw)
    nb, pb = n_pairs // per, (np.arange(n_pairs) // per).astype(np.int32)
    gidx, opt = lib.index_load(common.EXAMPLE_FA), lib.opt_init()
    keep = [to_dev(seq), to_dev(off), to_dev(pb)]
    _, dup = capi.hotpath_dev(lib, gidx, opt, n_pairs, read_len, keep[0][1], keep[1][1], keep[2][1], nb, 0, True)
    s16, h = capi.hotpath_dev_ex(lib, gidx, opt, n_pairs, read_len, keep[0][1], keep[1][1], keep[2][1], nb, 0, keep=True)
    res, bits, mate = capi.dev_records_download(lib, h, n_pairs)
    names = [nm for nm, _, _ in pairs for _ in (0, 1)]
    text, _ = capi.sam_format(lib, gidx, opt, res, names, seq, off, None, "")
    blocks = [R.record_lines(*p) for p in recs_of_result(res)]
    res.close(); capi.dev_records_free(lib, h)
    flat = [l for b in blocks for l in b]
    rows = [l.split("\t") for l in text.split("\n") if l]
    assert [(0 if f[2] == "20_slice" else -1, int(f[3]), int(f[1]), int(f[4]), f[5]) for f in rows] == [tuple(l) for l in flat]
    o = ropt(exclude_dups=1, add_mate_tags=1)                                                   # what the step runs with
    rdup = R.mark_duplicates(blocks)
    assert dup.tolist() == rdup
    left, base, c, r = {"Tie": 0, "Undefined": 0}, 0, [sum(rdup), 0, 0, len(flat)], [sum(rdup), 0, 0, len(flat)]      # c: the device's lines, r: the reference's
    for b, d in zip(blocks, rdup):
        got = bits[base:base + len(b)].tolist(), [int(m) - base if m >= 0 else -1 for m in mate[base:base + len(b)]]
        try:
            want = R.classify(b, d, o)
            assert got == want, (base, got, want)
            r[1] += sum(1 for x in want[0] if x & R.DISC); r[2] += sum(1 for x in want[0] if x & R.SPLIT)
        except (R.Tie, R.Undefined) as e:
            left[type(e).__name__] += 1
        c[1] += sum(1 for x in got[0] if x & R.DISC); c[2] += sum(1 for x in got[0] if x & R.SPLIT)
        base += len(b)
    n_left = sum(left.values())
    assert n_left * 100 <= len(blocks), left
    assert [int(s16[1]), int(s16[8]), int(s16[9]), int(s16[10])] == c                            # the step's counts are those of its own lines ...
    assert n_left or c == r                                                                     # ... and the reference's, where it decided every block
    assert r[0] > n_pairs // 40 and r[1] > 0 and (r[2] > 0 or n_pairs < 2000), r                 # the floors check_hotpath asserts of the oracle, here of the reference's verdicts alone
    lib.index_destroy(gidx)
    return dict(pairs=n_pairs, lines=r[3], duplicates=r[0], discordant_lines=r[1], splitter_lines=r[2], left_out=left)


@pytest.mark.parametrize("read_len", [150, 250])
def test_emu_simulated(emu_lib, read_len):
    SEEN["simulated %d" % read_len] = hold_simulated(emu_lib, 600, 200, read_len, to_host)


def test_emu_records(emu_lib):
    hold_records_group(emu_lib)


@pytest.mark.gpu
def test_gpu_records(gpu_lib):
    hold_records_group(gpu_lib)


def test_emu_lines_as_records(emu_lib):
    lines_as_records(emu_lib)


@pytest.mark.gpu
def test_gpu_lines_as_records(gpu_lib):
    lines_as_records(gpu_lib)


def lines_as_records(lib):
    """the constructed blocks that a pair's records can print (two reads, primaries first in each) once more through ssg_dbg_sbl_records"""
    n = 0
    for group in ("end_keys", "discordant", "splitters"):
        for c in cases_of(group):
            pairs = []
            for b in c.stream[0]:
                reads = ([], [])
                for l in b:
                    lead_ops = tuple((int(x), op) for x, op in re.findall(r"(\d+)([MIDSH])", l.cigar))
                    mapped = R.is_mapped(l)
                    reads[0 if l.flag & 0x40 else 1].append(R.Rec(True, l.contig if mapped else -1, l.pos - 1 if mapped else -1, l.flag & 0x8c2, l.mapq, 1 if l.flag & 0x10 and mapped else 0,
                                                                  lead_ops if mapped else ()))
                pairs.append(reads)
            blocks = [R.record_lines(*p) for p in pairs]
            sub = Case(c.name + " as records", [blocks], c.opt)
            hold_records(lib, pairs, sub)
            n += len(blocks)
    assert n > 60


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["owner", "simulated150", "simulated250"])
def test_gpu_with_device_buffers(gpu_lib, what):
    """ssg_markdup_sig_dev on every constructed stream and on raw equal-hash signatures; the simulated leg through ssg_hotpath_dev_ex (tests/sbl_check.py)"""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "sbl_check.py"), what], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sbl ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


def owner_side_everything(lib, to_dev):
    """what tests/sbl_check.py runs for `owner`: every constructed stream, the sizes and the raw equal-hash signatures through ssg_markdup_sig_dev"""
    for group in sorted(GROUPS):
        for c in cases_of(group):
            hold_owner_side(lib, [R.signature(b) for chunk in c.stream for b in chunk], to_dev, c.name)
    for n in SIZES:
        c = sizes_case(n)
        hold_owner_side(lib, c.sigs[0] if c.sigs else [R.signature(b) for b in c.stream[0]], to_dev, c.name)
    raw_equal_hash(lib, to_dev)


@pytest.fixture(scope="module", autouse=True)
def _write_counts():
    """with SBL_REFERENCE_COUNTS=path: what the groups run in this session reached, as JSON (how profiles/sbl_reference_counts.json is made)"""
    yield
    path = os.environ.get("SBL_REFERENCE_COUNTS")
    if path:
        import json
        with open(path, "w") as f:
            json.dump(SEEN, f, indent=1, sort_keys=True)


GROUPS = {"end_keys": group_end_keys, "blocks": group_blocks, "discordant": group_discordant, "splitters": group_splitters, "equal_hash_runs": group_equal_hash_runs}
_CASES = {}


def cases_of(group):
    if group not in _CASES:
        _CASES[group] = GROUPS[group]()
        SEEN.setdefault(group, {})["cases"] = {c.name: c.reached() for c in _CASES[group]}
    return _CASES[group]


def hold_pinned(lib, oracle):
    for name, stream, o, want_bits in pinned_cases():
        off, lines = to_arrays(stream[0])
        bits, _ = capi.sbl_process(lib, None, lopt(lib, o), off, lines)
        want = [x for w in want_bits for x in w]
        assert bits.tolist() == want, (name, bits.tolist())
        if oracle is not None:
            text = R.sam_text(stream[0])
            rm, rd, rs = common.sbl_streams_from_bits(text, want, [-1] * len(want), False, False)
            oracle.samblaster(R.sam_header(6) + text, exclude_dups=False, add_mate_tags=False, max_split=o.max_split_count, min_non_overlap=o.min_non_overlap)
            rec = lambda t: [l for l in t.split("\n") if l and l[0] != "@"]
            assert rec(oracle.last_discordants) == rd and rec(oracle.last_splitters) == rs, name


def hold_einval(lib):
    """--maxSplitCount above 16: refused on the host before any launch, by every form"""
    blocks = [split_block([piece(0, 1000, False, 0, 50, 100), piece(1, 1000, False, 50, 50, 100)], 0)]
    off, lines = to_arrays(blocks)
    o = lopt(lib, ropt(max_split_count=17))
    with pytest.raises(ValueError):
        R.classify(blocks[0], 0, ropt(max_split_count=17))
    with pytest.raises(capi.SsgError):
        capi.sbl_process(lib, None, o, off, lines)
    with pytest.raises(capi.SsgError):
        capi.sbl_classify(lib, o, off, lines, np.zeros(1, dtype=np.uint8))


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_emu_constructed(emu_lib, group):
    for c in cases_of(group):
        hold_lib(emu_lib, c)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_oracle_constructed(oracle, group):
    n = 0
    for c in cases_of(group):
        if c.oracle:                                                             # not the groups whose contig ids no header can hold
            hold_oracle(oracle, c); n += 1
    assert n or group == "equal_hash_runs"


def test_emu_pinned_choices_and_refusal(emu_lib, oracle):
    hold_pinned(emu_lib, oracle)
    hold_einval(emu_lib)
    raw_equal_hash(emu_lib, to_host)


@pytest.mark.parametrize("n", SIZES)
def test_emu_sizes(emu_lib, n):
    c = sizes_case(n)
    hold_lib(emu_lib, c)
    if os.environ.get("SBL_REFERENCE_COUNTS"):
        SEEN.setdefault("sizes", {})[str(n)] = c.reached() if c.sigs is None else dict(blocks=n, calls=1, duplicates=sum(c.ref()[0][0]))


@pytest.mark.parametrize("n", [n for n in SIZES if n <= 70001])
def test_oracle_sizes(oracle, n):
    hold_oracle(oracle, sizes_case(n))                                           # past 70001 pairs there are ends only, no lines to render


def test_oracle_records(oracle):
    hold_oracle(oracle, records_cases()[1])                                      # the lines R.record_lines makes of the records group


def test_oracle_table_growth(oracle):
    hold_oracle(oracle, table_cases("growth"))                                   # the one table stream whose contig ids a header can hold


@pytest.mark.parametrize("which", ["slot rule", "wrap", "growth", "contention"])
def test_emu_table(emu_lib, monkeypatch, which):
    monkeypatch.setenv("SSG_SBL_TABLE_SLOTS", "16")
    hold_lib(emu_lib, table_cases(which))


@pytest.mark.gpu
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_gpu_constructed(gpu_lib, group):
    for c in cases_of(group):
        hold_lib(gpu_lib, c, None)


@pytest.mark.gpu
def test_gpu_pinned_choices_and_refusal(gpu_lib):
    hold_pinned(gpu_lib, None)
    hold_einval(gpu_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_gpu_sizes(gpu_lib, n):
    hold_lib(gpu_lib, sizes_case(n), None)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["slot rule", "wrap", "growth", "contention"])
def test_gpu_table(gpu_lib, monkeypatch, which):
    monkeypatch.setenv("SSG_SBL_TABLE_SLOTS", "16")
    hold_lib(gpu_lib, table_cases(which), None)
