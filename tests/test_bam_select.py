"""Records selected on the device (k_bam_select.h; ssg_recs_select): a scanned chunk's records decided by a region list and a postfix filter program and the kept
ones compacted in stream order, against tests/view_reference.py -- a reference that shares no code with the product: it decodes the records with struct,
evaluates a filter by translating the expression's tokens to Python and tests overlap by its definition.  Every wave and workgroup edge of the compaction,
every edge of the overlap test and of the bisection, every operation of the filter, every refusal; and `sambamba view' with -F, -c, -o, -L and regions, on its
host path and with SSG_VIEW_DEVICE=1, against the same reference and against samtools 1.3.1.  CPU-side on the host emulation of the kernel; `-m gpu' on the MI355X."""
import ctypes as C
import functools
import gzip
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import view_reference as ref
from common import ROOT
from speedseq_amd import capi
from test_bam_scan import EOF_MARKER, OURS, load, reblock, rec, small_members, write_sam

SSG_EIO, SSG_EINVAL, SSG_EALIGN, SSG_EOVERFLOW = -5, -22, -71, -75
AB64 = 0xABABABABABABABAB


def fields(r, mapq=None, mtid=None, isize=None):
    """a record of rec() with other MAPQ, mate tid or template length"""
    b = bytearray(r)
    if mapq is not None:
        b[13] = mapq
    if mtid is not None:
        struct.pack_into("<i", b, 24, mtid)
    if isize is not None:
        struct.pack_into("<i", b, 32, isize)
    return bytes(b)


def group(recs, sizes=(3, 1, 2)):
    """the records as members' payloads of 3, 1, 2, 3, ... records: every member begins at a record"""
    out, i, k = [], 0, 0
    while i < len(recs):
        out.append(b"".join(recs[i:i + sizes[k % len(sizes)]]))
        i += sizes[k % len(sizes)]
        k += 1
    return out


class Chunk:
    """payloads loaded into a store, with the reference's view of the same bytes"""

    def __init__(self, lib, payloads, first=0):
        self.lib, self.first = lib, first
        self.recs, self.cid, self.off = load(lib, payloads)
        self.want = reference_of(b"".join(payloads), first)

    def select(self, regions=(), expr="", **kw):
        return capi.recs_select(self.lib, self.recs, self.cid, self.off, self.first, regions=regions, prog=ref.postfix(expr) if expr else (), **kw)

    def check(self, regions=(), expr="", sorted_regions=None):
        """the kept records equal the reference's, field by field and in order; the counting form agrees; returns the kept records' indices"""
        keep = ref.select(self.want, regions, expr)
        rc, n_rec, n_sel, loc, key, ent = self.select(sorted(regions) if sorted_regions is None else sorted_regions, expr)
        assert rc == 0, self.lib.l.ssg_last_error()
        assert n_rec == len(self.want) and n_sel == len(keep), (n_rec, n_sel, len(self.want), len(keep), regions, expr)
        want = [ref.loc_key_ent(self.want[i], self.cid) for i in keep]
        assert [int(x) for x in loc] == [w[0] for w in want]
        assert [int(x) for x in key] == [w[1] for w in want]
        assert [tuple(int(v) for v in e) for e in ent] == [w[2] for w in want]
        rc, n_rec2, n_sel2, _, _, _ = self.select(sorted(regions) if sorted_regions is None else sorted_regions, expr, counting=True)
        assert (rc, n_rec2, n_sel2) == (0, n_rec, n_sel)
        return keep

    def close(self):
        self.recs.close()


@functools.lru_cache(maxsize=None)
def reference_of(stream, first):
    return ref.records(stream, first)


# ---- the compaction: wave and workgroup edges, six selection patterns ----
PATTERNS = {"nothing": "supplementary", "everything": "", "every_second": "paired", "lane_0": "first_of_pair", "lane_63": "second_of_pair", "the_last": "failed_quality_control"}
COUNTS = ["1", "63", "64", "65", "255", "256", "257", "members_4097"]


@functools.lru_cache(maxsize=None)
def marked(name):
    """payloads whose records carry the patterns in their flags: 0x1 on every second record, 0x40 on lane 0 of a wave, 0x80 on lane 63, 0x200 on the last"""
    n = 4097 * 5 // 2 if name.startswith("members_") else int(name)
    sizes = (2, 3) if name.startswith("members_") else (3, 1, 2)
    if name.startswith("members_"):
        n = sum(sizes[k % 2] for k in range(4097))
    recs = []
    for i in range(n):
        flag = (0x1 if i % 2 else 0) | (0x40 if i % 64 == 0 else 0) | (0x80 if i % 64 == 63 else 0) | (0x200 if i == n - 1 else 0) | (0x10 if i % 5 == 0 else 0)
        recs.append(fields(rec(i % 3, 7 * i, flag, [(10 + i % 5, 0)], name=b"m%d\0" % i, l_seq=i % 4), mapq=i % 61, isize=i - 100))
    return group(recs, sizes)


def check_compaction(lib, name):
    payloads = marked(name)
    if name.startswith("members_"):
        assert len(payloads) == 4097
    c = Chunk(lib, payloads)
    n = len(c.want)
    assert name.startswith("members_") or n == int(name)
    rc, n_scan, _, _, _ = capi.recs_scan(lib, c.recs, c.cid, c.off, 0)
    assert rc == 0 and n_scan == n
    for pat, expr in PATTERNS.items():
        keep = c.check(expr=expr)
        want = {"nothing": [], "everything": list(range(n)), "every_second": list(range(1, n, 2)), "lane_0": list(range(0, n, 64)), "lane_63": list(range(63, n, 64)), "the_last": [n - 1]}[pat]
        assert keep == want, pat                                          # (the reference selects what the pattern is meant to be)
        if keep:                                                          # room for one record less: SSG_EOVERFLOW with both numbers and nothing written
            rc, n_rec, n_sel, loc, key, ent = c.select(expr=expr, cap=len(keep) - 1)
            assert rc == SSG_EOVERFLOW and n_rec == n and n_sel == len(keep)
            assert (loc == AB64).all() and (key == AB64).all() and ent.tobytes() == b"\xab" * ent.nbytes
    c.close()


@pytest.mark.parametrize("name", COUNTS)
def test_emu_compaction_is_stable_at_every_edge(emu_lib, name):
    check_compaction(emu_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", COUNTS)
def test_gpu_compaction_is_stable_at_every_edge(gpu_lib, name):
    check_compaction(gpu_lib, name)


# ---- the overlap test ----
END29 = 1 << 29
EDGE_REGIONS = [(0, 1000, 2000), (0, 3000, 3100), (0, 3200, 3300), (2, 0, 1), (2, END29 - 100, END29)]
EDGE_RECORDS = [   # name, in or out, the record
    (b"end_at_beg", False, rec(0, 900, 0, [(100, 0)])),
    (b"end_at_beg_plus_1", True, rec(0, 900, 0, [(101, 0)])),
    (b"pos_at_end_minus_1", True, rec(0, 1999, 0, [(10, 0)])),
    (b"pos_at_end", False, rec(0, 2000, 0, [(10, 0)])),
    (b"no_reference_at_beg", False, rec(0, 1000, 0, [(5, 4)])),
    (b"no_reference_inside", True, rec(0, 1500, 0, [(5, 4)])),
    (b"unmapped_last_base", True, rec(0, 1999, 4, [])),
    (b"unmapped_before_beg", False, rec(0, 999, 4, [])),
    (b"unmapped_ignores_cigar", False, rec(0, 999, 4, [(50, 0)])),
    (b"no_tid", False, rec(-1, 1500, 4, [])),
    (b"no_tid_mapped_flag", False, rec(-1, 1500, 0, [(10, 0)])),
    (b"tid_without_region", False, rec(1, 1500, 0, [(10, 0)])),
    (b"spans_two_regions", True, rec(0, 3050, 0, [(200, 0)])),
    (b"between_two_regions", False, rec(0, 3100, 0, [(100, 0)])),
    (b"covers_everything", True, rec(0, 0, 0, [(5000, 0)])),
    (b"first_base", True, rec(2, 0, 0, [(1, 0)])),
    (b"second_base", False, rec(2, 1, 0, [(1, 0)])),
    (b"last_base_of_2_29", True, rec(2, END29 - 1, 0, [(1, 0)])),
    (b"ends_at_last_region", False, rec(2, END29 - 150, 0, [(50, 0)])),
    (b"reaches_last_region", True, rec(2, END29 - 150, 0, [(30, 0), (5, 2), (16, 0)])),
    (b"behind_every_region", False, rec(3, 5, 0, [(10, 0)])),
    (b"position_minus_1", False, rec(0, -1, 0, [(10, 0)])),
]


def edge_payloads():
    return group([rec_named(r, n) for n, _, r in EDGE_RECORDS])


def rec_named(r, name):
    """the record with another read name (rec() gives every record the name "r")"""
    l_qname = r[12]
    body = bytearray(r[4:12] + bytes([len(name) + 1]) + r[13:36] + name + b"\0" + r[36 + l_qname:])
    return struct.pack("<I", len(body)) + bytes(body)


def check_overlap_edges(lib):
    c = Chunk(lib, edge_payloads())
    keep = c.check(regions=EDGE_REGIONS)
    assert [c.want[i]["name"] for i in keep] == [n for n, inside, _ in EDGE_RECORDS if inside]
    # a region list in another order is refused, not sorted: the caller merges and sorts
    rc, _, _, _, _, _ = c.select(EDGE_REGIONS[::-1])
    assert rc == SSG_EINVAL
    # every region alone, and with a filter behind it
    for g in EDGE_REGIONS:
        c.check(regions=[g])
        c.check(regions=[g], expr="not unmapped")
    c.close()


def test_emu_overlap_edges(emu_lib):
    check_overlap_edges(emu_lib)


@pytest.mark.gpu
def test_gpu_overlap_edges(gpu_lib):
    check_overlap_edges(gpu_lib)


def test_the_overlap_cases_are_what_they_are_meant_to_be():
    want = ref.records(b"".join(edge_payloads()))
    by = {r["name"]: r for r in want}
    assert len(by) == len(EDGE_RECORDS)
    assert by[b"end_at_beg"]["end"] == 1000 and by[b"end_at_beg_plus_1"]["end"] == 1001 and by[b"no_reference_at_beg"]["end"] == by[b"no_reference_at_beg"]["pos"] == 1000
    assert by[b"unmapped_last_base"]["end"] == 2000 and by[b"unmapped_ignores_cigar"]["end"] == 1000 and by[b"reaches_last_region"]["end"] == END29 - 99
    keep = ref.select(want, EDGE_REGIONS)
    assert [want[i]["name"] for i in keep] == [n for n, inside, _ in EDGE_RECORDS if inside]
    assert 0 < len(keep) < len(want)


REGION_COUNTS = (1, 2, 64, 65, 1000)


@functools.lru_cache(maxsize=None)
def ladder_payloads():
    """records every 67 bases of contigs 0 and 1, each 10 to 40 bases long"""
    recs = [rec(t, 67 * i, 16 if i % 3 == 0 else 0, [(10 + i % 31, 0)], name=b"l%d\0" % i) for t in (0, 1) for i in range(1500)]
    return group(recs)


def ladder_regions(n):
    """n regions of 50 bases every 100 on contig 0, the last third of them on contig 1"""
    return [(0 if k < n - n // 3 else 1, 100 * k, 100 * k + 50) for k in range(n)]


def check_region_counts(lib):
    c = Chunk(lib, ladder_payloads())
    for n in REGION_COUNTS:
        keep = c.check(regions=ladder_regions(n))
        assert 0 < len(keep) < len(c.want)
    c.close()


def test_emu_bisection_depths(emu_lib):
    check_region_counts(emu_lib)


@pytest.mark.gpu
def test_gpu_bisection_depths(gpu_lib):
    check_region_counts(gpu_lib)


# ---- the filter program ----
@functools.lru_cache(maxsize=None)
def filter_payloads():
    recs = []
    for k in range(12):                                                   # every flag bit alone, and all but it
        recs.append(rec(0, 100 + k, 1 << k, [(10, 0)], name=b"f%d\0" % k))
        recs.append(rec(0, 200 + k, 0xfff ^ 1 << k, [(10, 0)], name=b"g%d\0" % k))
    recs.append(rec(0, 300, 0, [(10, 0)]))
    recs.append(rec(0, 301, 0xfff, [(10, 0)]))
    k = 0
    for mapq in (0, 19, 20, 21, 254, 255):
        for isize in (-501, -500, -499, 0, 499, 500, 501):
            recs.append(fields(rec(k % 4 - 1, 400 + k, (99, 147, 1024 | 83, 4)[k % 4], [(10, 0)] if k % 4 < 3 else [], l_seq=(0, 9, 10, 11, 12)[k % 5]), mapq=mapq, mtid=(k // 2) % 4 - 1, isize=isize))
            k += 1
    return group(recs)


FIELD_VALUES = {"mapping_quality": 20, "ref_id": 1, "mate_ref_id": 1, "template_length": -500, "sequence_length": 10, "flag": 99}


def wide_expression():
    """32 pushes joined by 31 alternating and / or with a `not' in front: a program of exactly 64 operations (flat: the stack never holds more than two values)"""
    terms = ["%s" % n for n in ref.FLAGS] + ["mapping_quality >= %d" % v for v in (1, 20, 21, 255)] + ["template_length < %d" % v for v in (-500, 0, 500, 501)]
    terms += ["ref_id == 1", "mate_ref_id != 1", "sequence_length > 9", "sequence_length <= 10"] + ["flag == %d" % v for v in (99, 147, 4, 0)] + ["ref_id >= 0", "ref_id < 2", "mate_ref_id >= 1", "flag != 99"]
    assert len(terms) == 32
    flat = terms[0]
    for k, t in enumerate(terms[1:]):
        flat = "(%s %s %s)" % (flat, "or" if k % 2 else "and", t)
    deep = terms[-1]
    for k, t in enumerate(terms[-2::-1]):
        deep = "(%s %s %s)" % (t, "or" if k % 3 else "and", deep)
    return "not " + flat, "not " + deep


def check_filter(lib):
    c = Chunk(lib, filter_payloads())
    n = len(c.want)
    for name in ref.FLAGS:
        a, b = c.check(expr=name), c.check(expr="not " + name)
        assert sorted(a + b) == list(range(n)) and a and b
    for field, v in FIELD_VALUES.items():
        for cmp in ref.CMPS:
            for d in (-1, 0, 1):
                c.check(expr="%s %s %d" % (field, cmp, v + d))
    assert c.check(expr="mapping_quality == 0") and c.check(expr="mapping_quality >= 255") and c.check(expr="mapping_quality > 255") == [] and c.check(expr="mapping_quality < 0") == []
    assert len(c.check(expr="mapping_quality <= 255")) == n
    assert c.check(expr="template_length < -500") and c.check(expr="template_length == -500") and c.check(expr="template_length < 0 and template_length > -501")
    assert c.check(expr="mate_ref_id == -1") and c.check(expr="ref_id < 0")
    x = "proper_pair and mapping_quality >= 20"
    assert c.check(expr="not not (%s)" % x) == c.check(expr=x) and c.check(expr="not (%s)" % x) == c.check(expr="not not not (%s)" % x)
    assert c.check(expr="proper_pair and not duplicate and mapping_quality >= 20")
    assert c.check(expr="unmapped or duplicate and not reverse_strand or template_length > 500")
    # exactly 64 operations, flat and nested as deep as 64 operations can nest: 32 values on the stack
    flat, deep = wide_expression()
    for e in (flat, deep):
        prog = ref.postfix(e)
        assert len(prog) == 64
        c.check(expr=e)
        c.check(expr=e[4:])
    depth = most = 0
    for op, _, _ in ref.postfix(deep):
        depth += -1 if op in (1, 2) else 0 if op == 3 else 1
        most = max(most, depth)
    assert most == 32
    # with a region in front
    c.check(regions=[(0, 205, 210), (1, 0, 420)], expr="not unmapped and mapping_quality >= 20")
    c.close()


def test_emu_filter_program(emu_lib):
    check_filter(emu_lib)


@pytest.mark.gpu
def test_gpu_filter_program(gpu_lib):
    check_filter(gpu_lib)


# ---- refusals ----
PUSH, AND, NOT = (capi.FOP_FLAG, 0, 1), (capi.FOP_AND, 0, 0), (capi.FOP_NOT, 0, 0)
BAD_ARGS = [   # what, regions, program, the message's words
    ("unsorted regions", [(0, 100, 200), (0, 10, 20)], [], rb"region 1 is not behind region 0"),
    ("regions of descending tid", [(1, 10, 20), (0, 10, 20)], [], rb"region 1 is not behind region 0"),
    ("overlapping regions", [(0, 10, 20), (0, 19, 30)], [], rb"region 1 is not behind region 0"),
    ("touching regions", [(0, 10, 20), (0, 20, 30)], [], rb"region 1 is not behind region 0"),
    ("an empty region", [(0, 10, 10)], [], rb"region 0 has .*beg >= end"),
    ("a reversed region", [(0, 10, 20), (0, 40, 30)], [], rb"region 1 has .*beg >= end"),
    ("a region without contig", [(-1, 10, 20)], [], rb"region 0 has tid < 0"),
    ("65 operations", [], [PUSH] + [NOT] * 64, rb"65 operations, at most 64"),
    ("and on one value", [], [PUSH, AND], rb"operation 1 underflows the stack"),
    ("not on nothing", [], [NOT, PUSH], rb"operation 0 underflows the stack"),
    ("two values left", [], [PUSH, PUSH], rb"leaves 2 values"),
    ("an unknown operation", [], [PUSH, (10, 0, 0), AND], rb"operation 1 is the unknown operation 10"),
    ("an unknown field", [], [(capi.FOP_GE, 6, 0)], rb"operation 0 compares the unknown field 6"),
]


def check_refusals(lib):
    c = Chunk(lib, marked("65"))
    for what, regions, prog, words in BAD_ARGS:
        rc, n_rec, n_sel, loc, key, ent = capi.recs_select(lib, c.recs, c.cid, c.off, 0, regions=regions, prog=prog)
        msg = lib.l.ssg_last_error()
        assert rc == SSG_EINVAL and msg.startswith(b"ssg_recs_select: ") and re.search(words, msg), (what, rc, msg)
        assert (n_rec, n_sel) == (0, 0) and (loc == AB64).all() and (key == AB64).all() and ent.tobytes() == b"\xab" * ent.nbytes, what
        assert c.check(expr="paired") == list(range(1, 65, 2)), what          # the store is usable afterwards
    # two regions that are one base apart, and 64 operations, are taken
    assert capi.recs_select(lib, c.recs, c.cid, c.off, 0, regions=[(0, 10, 20), (0, 21, 30)], prog=[PUSH] + [NOT] * 63)[0] == 0
    # arrays without room and room without arrays
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    n_rec, n_sel, one = C.c_uint64(7), C.c_uint64(7), np.zeros(1, dtype=np.uint64)
    head = (c.recs.h, C.c_uint32(c.cid), ptr(c.off), C.c_int64(len(c.off) - 1), C.c_uint64(0), None, C.c_int64(0), None, C.c_int(0))
    assert lib.l.ssg_recs_select(*head, C.c_uint64(65), C.byref(n_rec), C.byref(n_sel), None, None, None) == SSG_EINVAL and b"counting form" in lib.l.ssg_last_error()
    assert lib.l.ssg_recs_select(*head, C.c_uint64(65), C.byref(n_rec), C.byref(n_sel), ptr(one), None, None) == SSG_EINVAL
    assert lib.l.ssg_recs_select(*head, C.c_uint64(65), None, C.byref(n_sel), None, None, None) == SSG_EINVAL
    # a chunk that does not exist: the scan's refusal, under this entry's name
    rc = capi.recs_select(lib, c.recs, 5, c.off, 0)[0]
    assert rc == SSG_EINVAL and lib.l.ssg_last_error() == b"ssg_recs_select: chunk 5 does not exist or is released"
    # refused while an order is declared; taken again after ssg_recs_reopen
    rc, n, loc, key, ent = capi.recs_scan(lib, c.recs, c.cid, c.off, 0)
    capi.recs_order(lib, c.recs, loc, np.concatenate([[0], np.cumsum(ent["len"].astype(np.uint64))]).astype(np.uint64))
    rc = c.select(expr="paired")[0]
    assert rc == SSG_EINVAL and b"while an order is declared" in lib.l.ssg_last_error()
    capi.recs_reopen(lib, c.recs)
    assert len(c.check(expr="paired")) == 32
    c.close()


def test_emu_select_refuses_bad_regions_and_programs(emu_lib):
    check_refusals(emu_lib)


@pytest.mark.gpu
def test_gpu_select_refuses_bad_regions_and_programs(gpu_lib):
    check_refusals(gpu_lib)


def check_bad_streams(lib):
    """the misaligned and the malformed streams of test_bam_scan.py: the scan's code and the scan's words"""
    p = small_members(4, 31)
    stream = b"".join(p)
    a, b = len(p[0]), len(p[0]) + len(p[1]) + len(p[2]) - 11             # member 2 begins inside a record
    recs, cid, off = load(lib, [stream[:a], stream[a:b], stream[b:]], cap=len(stream))
    rc, n_rec, n_sel, loc, key, ent = capi.recs_select(lib, recs, cid, off, 0, prog=[PUSH])
    msg = lib.l.ssg_last_error()
    rc2 = capi.recs_scan(lib, recs, cid, off, 0)[0]
    assert rc == rc2 == SSG_EALIGN and msg.split(b": ", 1)[1] == lib.l.ssg_last_error().split(b": ", 1)[1] and re.search(rb"not record-aligned at hint 1\b", msg), msg
    assert n_sel == 0 and (loc == AB64).all() and (key == AB64).all() and ent.tobytes() == b"\xab" * ent.nbytes
    rc, n_rec, n_sel, loc, key, ent = capi.recs_select(lib, recs, cid, [0, len(stream)], 0)   # the one hint that holds: the whole stream
    assert rc == 0 and n_rec == n_sel == len(ref.records(stream))
    recs.close()
    p = small_members(6, 37)
    good = b"".join(p)
    at = len(p[0]) + len(p[1])
    cuts = [0] + list(np.cumsum([len(x) for x in p]))
    last = ref.records(good)[-1]["off"]
    bs, = struct.unpack_from("<I", good, at)
    for where, word, words in ((at, 31, b"below 32"), (last, len(good) - last - 4 + 1, b"past the end"), (last, 0xffffffff, b"past the end"), (at + 16, bs // 4 + 1, b"n_cigar")):
        bad = bytearray(good)
        struct.pack_into("<I", bad, where, word)
        recs, cid, off = load(lib, [bytes(bad)[x:y] for x, y in zip(cuts[:-1], cuts[1:])])
        rc, n_rec, n_sel, loc, key, ent = capi.recs_select(lib, recs, cid, off, 0, regions=[(0, 0, 1 << 20)], prog=[PUSH])
        msg = lib.l.ssg_last_error()
        rc2 = capi.recs_scan(lib, recs, cid, off, 0)[0]
        assert rc == rc2 == SSG_EIO and words in msg and msg.split(b": ", 1)[1] == lib.l.ssg_last_error().split(b": ", 1)[1], msg
        assert n_sel == 0 and (loc == AB64).all()
        rc, _, n_sel, _, _, _ = capi.recs_select(lib, recs, cid, off, 0, counting=True)
        assert rc == SSG_EIO and n_sel == 0                               # the counting form reads the same stream
        recs.close()


def test_emu_select_reports_bad_streams_as_the_scan_does(emu_lib):
    check_bad_streams(emu_lib)


@pytest.mark.gpu
def test_gpu_select_reports_bad_streams_as_the_scan_does(gpu_lib):
    check_bad_streams(gpu_lib)


# ---------------- sambamba view -F / -c / -o ----------------
SAMTOOLS = os.path.join(ROOT, "oracle", "_ref", "samtools")
VIEW_DEV = {"SSG_VIEW_DEVICE": "1"}
# name -> (filter or None, the samtools arguments that select the same records or None)
QUERIES = {
    "count_alone": (None, ()),
    "usual": ("proper_pair and not duplicate and mapping_quality >= 20", ("-f", "2", "-F", "1024", "-q", "20")),
    "mapped": ("not unmapped", ("-F", "4")),                                  # the unmapped tail excluded
    "unmapped": ("unmapped", ("-f", "4")),
    "reverse_floor": ("reverse_strand and not (secondary_alignment or supplementary) and mapping_quality >= 21", ("-f", "16", "-F", "2304", "-q", "21")),
    "one_contig": ("ref_id == 1 and mate_ref_id == 1", None),
    "lengths": ("template_length < 0 or mapping_quality == 0 and sequence_length >= 100", None),
    "flag_value": ("flag == 99 or flag == 147", None),
    "nothing": ("supplementary and unmapped", ("-f", "2052")),               # the one query that keeps no record
}


def vary(path, seed):
    """the SAM file of write_sam with other flags, mapping qualities and mates on its mapped records"""
    rng = np.random.RandomState(seed)
    out = []
    for l in open(path).read().split("\n"):
        c = l.split("\t")
        if l and not l.startswith("@") and c[2] != "*":
            c[1] = str(int(rng.choice([0, 16, 99, 147, 83, 163, 1024 | 99, 1024 | 147, 65, 2048 | 16, 256, 512 | 99])))
            c[4] = str(int(rng.choice([0, 5, 19, 20, 21, 60])))
            if int(c[1]) & 1:
                c[6], c[7], c[8] = "=", str(int(c[3]) + 150), str(250 if int(c[1]) & 32 else -250)
        out.append("\t".join(c))
    open(path, "w").write("\n".join(out))


# records at known places (three each, 100M): the first base of a 1-base query, a 16 kb window's edge, the last bases of two contigs
PLACED = [("ctgA", 1000, 0), ("ctgA", 16350, 16), ("ctgB", 249901, 0), ("ctgC", 89000, 16)]


class Viewer:
    """a coordinate-sorted BAM of about 2200 records over three contigs made through the product's own view and sort, as the sort wrote it and in blocks of about 20 kB
    that start at records (some tens of members), and every run of `view' on them"""

    def __init__(self, sambamba, d):
        self.sambamba, self.d, self.runs = sambamba, str(d), {}
        self.clean = {k: v for k, v in os.environ.items() if k not in OURS + ("SSG_VIEW_DEVICE", "SSG_VIEW_POOL", "SSG_BGZF_DEVICE_LEVELS", "SSG_PROF")}
        write_sam(self.d + "/in.sam", 11, 2000, 200, PLACED, "gv")
        vary(self.d + "/in.sam", 12)
        with open(self.d + "/in.sam", "rb") as fi, open(self.d + "/in.u.bam", "wb") as fo:
            subprocess.run([sambamba, "view", "-S", "-f", "bam", "/dev/stdin"], stdin=fi, stdout=fo, check=True, env=self.clean)
        subprocess.run([sambamba, "sort", "-t", "4", "-m", "1G", "--tmpdir=%s/tmp" % self.d, "-o", self.d + "/sorted.bam", self.d + "/in.u.bam"], check=True, capture_output=True, env=self.clean)
        bam = open(self.d + "/sorted.bam", "rb").read()
        open(self.d + "/blocks.bam", "wb").write(reblock(bam))
        open(self.d + "/skew.bam", "wb").write(reblock(bam, step=3001))
        for name in ("sorted", "blocks", "skew"):                                         # every form indexed by the product's own `sambamba index'
            for x in (".bai", ".bai.ssg"):
                if os.path.exists("%s/%s.bam%s" % (self.d, name, x)):
                    os.remove("%s/%s.bam%s" % (self.d, name, x))
            subprocess.run([sambamba, "index", "-t", "4", "%s/%s.bam" % (self.d, name)], check=True, capture_output=True, env=self.clean)
        self.header, self.refs, self.records = ref.read_bam(self.d + "/sorted.bam")
        self.lines = self.run("whole", ["sorted.bam"], {}).stdout.split(b"\n")[:-1]   # the product's own BAM to SAM printer on the whole file
        assert len(self.lines) == len(self.records) == 2200 + 3 * len(PLACED)

    def run(self, tag, args, extra, stdin=None):
        if tag not in self.runs:
            env = dict(self.clean, SSG_DEBUG="1")
            env.update(extra)
            r = subprocess.run([self.sambamba, "view", "-t", "4"] + [self.d + "/" + a if a.endswith((".bam", ".sam")) and "/" not in a else a for a in args], capture_output=True, env=env, input=stdin)
            r.stderr = r.stderr.decode()
            self.runs[tag] = r
        return self.runs[tag]

    def kept(self, expr):
        return ref.select(self.records, (), expr or "")


@pytest.fixture(scope="module")
def emu_viewer(tmp_path_factory, emu_lib):
    return Viewer(os.path.join(ROOT, "tests", "emu", "sambamba_emu"), tmp_path_factory.mktemp("bam_select_emu"))


@pytest.fixture(scope="module")
def gpu_viewer(tmp_path_factory, gpu_lib):
    return Viewer(os.path.join(ROOT, "bin", "sambamba"), tmp_path_factory.mktemp("bam_select_gpu"))


def check_query(v, name):
    expr, _ = QUERIES[name]
    keep = v.kept(expr)
    want = b"".join(v.lines[i] + b"\n" for i in keep)
    flt = ["-F", expr] if expr else []
    for bam in ("sorted.bam", "blocks.bam"):
        outs = {}
        for how, extra in (("host", {}), ("dev", VIEW_DEV)):
            # (the device counts in the file as the sort wrote it and prints from the one of many members: a process that opens the GPU takes most of a second)
            sam = bool(expr) and (how == "host" or bam == "blocks.bam")
            if not sam:
                r = v.run("%s_%s_%s_c" % (name, bam, how), ["-c"] + flt + [bam], extra)
                assert r.returncode == 0 and r.stdout == b"%d\n" % len(keep), (how, r.stdout, r.stderr[-2000:])
            else:
                r = v.run("%s_%s_%s" % (name, bam, how), flt + [bam], extra)
                assert r.returncode == 0 and r.stdout == want, (how, r.stderr[-2000:])    # the selected line numbers of the whole file's text, line for line
                if how == "host":
                    assert v.run("%s_%s_%s_c" % (name, bam, how), ["-c"] + flt + [bam], extra).stdout == b"%d\n" % len(keep)
            outs[how] = r
            if how == "dev":
                line = re.findall(r"view: on the device: (\d+) of (\d+) members read, (\d+) records scanned, (\d+) kept, (\d+) batches", r.stderr)
                assert len(line) == 1 and "device view off" not in r.stderr, r.stderr[-2000:]
                assert (int(line[0][2]), int(line[0][3])) == (len(v.records), len(keep)) and (bam == "sorted.bam" or int(line[0][0]) > 10)
            else:
                assert "device" not in r.stderr
        assert bam == "sorted.bam" and expr or outs["host"].stdout == outs["dev"].stdout   # byte-equal (in the first file the device run of a filter only counts)
    if name == "usual":   # -h puts the header in front; -o writes the same bytes to a file
        for how, extra in (("host", {}), ("dev", VIEW_DEV)):
            out = "%s/o_%s_%s.sam" % (v.d, name, how)
            r = v.run("%s_%s_o" % (name, how), ["-h", "-o", out] + flt + ["blocks.bam"], extra)
            assert r.returncode == 0 and r.stdout == b"" and open(out, "rb").read() == v.header[8:8 + struct.unpack_from("<i", v.header, 4)[0]].rstrip(b"\0") + want, r.stderr[-2000:]


@pytest.mark.parametrize("name", sorted(QUERIES))
def test_emu_view_filters_and_counts(emu_viewer, name):
    check_query(emu_viewer, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(QUERIES))
def test_gpu_view_filters_and_counts(gpu_viewer, name):
    check_query(gpu_viewer, name)


def test_the_queries_are_what_they_are_meant_to_be(emu_viewer):
    """every query but the named empty one and the count of the whole file keeps at least one record and fewer than all of them"""
    n = len(emu_viewer.records)
    for name, (expr, _) in QUERIES.items():
        k = len(emu_viewer.kept(expr))
        assert (k == 0) if name == "nothing" else (k == n) if name == "count_alone" else (0 < k < n), (name, k)
    assert len(emu_viewer.kept("unmapped")) == 200 and len({r["tid"] for r in emu_viewer.records}) == 4
    assert len(gzip_members(open(emu_viewer.d + "/blocks.bam", "rb").read())) > 20


# name -> (the regions as they are typed, or the lines of a BED file; the same 0-based half-open on (tid, beg, end); a filter or None; samtools' arguments or None)
BIG = (1 << 31) - 1
REGION_QUERIES = {
    "whole_contig": (["ctgB"], [(1, 0, BIG)], None, ("ctgB",)),
    "one_base": (["ctgA:1000-1000"], [(0, 999, 1000)], None, ("ctgA:1000-1000",)),
    "inside_a_window": (["ctgA:20,000-23,000"], [(0, 19999, 23000)], None, ("ctgA:20000-23000",)),
    "across_a_window_edge": (["ctgA:16,300-16,500"], [(0, 16299, 16500)], None, ("ctgA:16300-16500",)),
    "last_base": (["ctgB:250000"], [(1, 249999, BIG)], None, ("ctgB:250000",)),
    "last_base_closed": (["ctgB:250,000-250,000"], [(1, 249999, 250000)], None, ("ctgB:250000-250000",)),
    "two_overlapping": (["ctgA:1000-50000", "ctgA:30000-90000"], [(0, 999, 50000), (0, 29999, 90000)], None, None),
    "three_descending": (["ctgC:100-20000", "ctgA:300000-310000", "ctgA:5000-16000"], [(2, 99, 20000), (0, 299999, 310000), (0, 4999, 16000)], None, None),
    "three_by_bed": ("#a comment\ntrack name=x\nbrowser position ctgA:1-2\nctgC\t99\t20000\tname\nctgA 299999 310000\n\nctgA\t4999\t16000\n", [(2, 99, 20000), (0, 299999, 310000), (0, 4999, 16000)], None, None),
    "touching": (["ctgA:1000-2000", "ctgA:2001-3000", "ctgA:2900-3100"], [(0, 999, 3100)], None, ("ctgA:1000-3100",)),
    "with_filter": (["ctgA:1-200000"], [(0, 0, 200000)], "proper_pair and not duplicate and mapping_quality >= 20", ("-f", "2", "-F", "1024", "-q", "20", "ctgA:1-200000")),
    "no_record": (["ctgC:91,000-92,000"], [(2, 90999, 92000)], None, ("ctgC:91000-92000",)),       # no record reaches it (the longest ends at 90 899)
    "behind_the_contig": (["ctgC:95000"], [(2, 94999, BIG)], None, None),
}


SMALL = ("one_base", "inside_a_window", "across_a_window_edge", "last_base", "last_base_closed", "no_record", "behind_the_contig")


def check_region_query(v, name):
    typed, regions, expr, _ = REGION_QUERIES[name]
    keep = ref.select(v.records, regions, expr or "")
    want = b"".join(v.lines[i] + b"\n" for i in keep)
    if isinstance(typed, str):
        open("%s/%s.bed" % (v.d, name), "w").write(typed)
    for bam in ("sorted.bam", "blocks.bam"):
        args = (["-F", expr] if expr else []) + (["-L", "%s/%s.bed" % (v.d, name), bam] if isinstance(typed, str) else [bam] + typed)
        for how, extra in (("host", {}), ("dev", VIEW_DEV)):
            if how == "host" or bam == "sorted.bam":
                r = v.run("%s_%s_%s_c" % (name, bam, how), ["-c"] + args, extra)
                assert r.returncode == 0 and r.stdout == b"%d\n" % len(keep), (how, r.stdout, r.stderr[-2000:])
            if how == "host" or bam == "blocks.bam":
                r = v.run("%s_%s_%s" % (name, bam, how), args, extra)
                assert r.returncode == 0 and r.stdout == want, (how, r.stderr[-2000:])
            if how == "dev":
                line = re.findall(r"view: on the device: (\d+) of (\d+) members read, (\d+) records scanned, (\d+) kept", r.stderr)
                assert len(line) == 1 and "device view off" not in r.stderr and int(line[0][3]) == len(keep), r.stderr[-2000:]
                read, have = int(line[0][0]), int(line[0][1])
                assert have == len(gzip_members(open(v.d + "/" + bam, "rb").read())) and read <= have
                if bam == "blocks.bam" and name in SMALL:                     # the index is really used: a small region leaves most of the file unread
                    assert read < have and int(line[0][2]) < len(v.records), line


@pytest.mark.parametrize("name", sorted(REGION_QUERIES))
def test_emu_view_regions(emu_viewer, name):
    check_region_query(emu_viewer, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(REGION_QUERIES))
def test_gpu_view_regions(gpu_viewer, name):
    check_region_query(gpu_viewer, name)


def test_the_region_queries_are_what_they_are_meant_to_be(emu_viewer):
    v, n = emu_viewer, len(emu_viewer.records)
    for name, (typed, regions, expr, _) in REGION_QUERIES.items():
        k = len(ref.select(v.records, regions, expr or ""))
        assert (k == 0) if name in ("no_record", "behind_the_contig") else (0 < k < n), (name, k)
    one = ref.select(v.records, REGION_QUERIES["one_base"][1])
    assert sum(1 for i in one if v.records[i]["pos"] == 999) == 3                      # the three records placed there, and whatever else covers the base
    assert ref.select(v.records, REGION_QUERIES["three_descending"][1]) == ref.select(v.records, REGION_QUERIES["three_by_bed"][1])
    both = ref.select(v.records, REGION_QUERIES["two_overlapping"][1])
    assert len(both) == len(set(both)) < len(ref.select(v.records, [(0, 999, 50000)])) + len(ref.select(v.records, [(0, 29999, 90000)]))   # the union: every record once


def check_regions_against_samtools(v):
    """samtools 1.3.1 with the file's index names the same records for every single-region query (none may be skipped: without the binary this fails)"""
    assert os.path.exists(SAMTOOLS), "oracle/_ref/samtools is not built"
    bam = v.d + "/st.bam"
    if not os.path.exists(bam + ".bai"):
        open(bam, "wb").write(open(v.d + "/sorted.bam", "rb").read())
        subprocess.run([SAMTOOLS, "index", bam], check=True)
    for name, (typed, regions, expr, args) in sorted(REGION_QUERIES.items()):
        if args is None:
            continue
        opts, where = [a for a in args if ":" not in a and not a.startswith("ctg")], [a for a in args if ":" in a or a.startswith("ctg")]
        cnt = subprocess.run([SAMTOOLS, "view", "-c"] + opts + [bam] + where, capture_output=True, check=True).stdout
        names = [l.split(b"\t")[0] for l in subprocess.run([SAMTOOLS, "view"] + opts + [bam] + where, capture_output=True, check=True).stdout.split(b"\n")[:-1]]
        for tag in ("sorted.bam_host", "blocks.bam_dev"):
            assert [l.split(b"\t")[0] for l in v.runs["%s_%s" % (name, tag)].stdout.split(b"\n")[:-1]] == names, (name, tag)
        assert v.runs["%s_sorted.bam_host_c" % name].stdout == v.runs["%s_sorted.bam_dev_c" % name].stdout == cnt, name


def test_emu_view_regions_agree_with_samtools(emu_viewer):
    for name in REGION_QUERIES:
        check_region_query(emu_viewer, name)
    check_regions_against_samtools(emu_viewer)


@pytest.mark.gpu
def test_gpu_view_regions_agree_with_samtools(gpu_viewer):
    for name in REGION_QUERIES:
        check_region_query(gpu_viewer, name)
    check_regions_against_samtools(gpu_viewer)


# BAM to BAM: name -> (what is typed behind the options, the regions 0-based half-open, a filter or None, -l or None)
BAM_QUERIES = {
    "whole_file": ([], [], None, None),
    "filter": ([], [], "proper_pair and not duplicate and mapping_quality >= 20", None),
    "contig": (["ctgB"], [(1, 0, BIG)], None, "9"),
    "small_region": (["ctgA:16,300-16,500"], [(0, 16299, 16500)], None, "1"),
    "regions_and_filter": (["ctgC:100-20000", "ctgA:5000-16000"], [(2, 99, 20000), (0, 4999, 16000)], "not unmapped and mapping_quality >= 20", None),
    "nothing": (["ctgC:91,000-92,000"], [(2, 90999, 92000)], None, None),
}


def check_bam_out(v, name):
    """-f bam: the inflated payload is the header and exactly the selected records, the file ends in the end-of-file marker, samtools counts the same"""
    typed, regions, expr, level = BAM_QUERIES[name]
    keep = ref.select(v.records, regions, expr or "")
    want = v.header + b"".join(v.records[i]["bytes"] for i in keep)
    assert os.path.exists(SAMTOOLS), "oracle/_ref/samtools is not built"
    for bam in ("sorted.bam", "blocks.bam"):
        for how, extra in (("host", {}), ("dev", dict(VIEW_DEV, SSG_BGZF_DEVICE_LEVELS="1"))):
            if how == "dev" and bam == "sorted.bam" and name != "whole_file":
                continue
            out = "%s/bo_%s_%s_%s" % (v.d, name, how, bam)
            r = v.run("bo_%s_%s_%s" % (name, bam, how), ["-f", "bam"] + (["-l", level] if level else []) + (["-F", expr] if expr else []) + ["-o", out, bam] + typed, extra)
            assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
            data = open(out, "rb").read()
            assert gzip.decompress(data) == want and data.endswith(EOF_MARKER) and not data[:-28].endswith(EOF_MARKER), (name, bam, how)
            assert all(struct.unpack_from("<I", data, o + struct.unpack_from("<H", data, o + 16)[0] + 1 - 4)[0] <= 0xff00 for o in gzip_members(data))
            assert subprocess.run([SAMTOOLS, "view", "-c", out], capture_output=True, check=True).stdout == b"%d\n" % len(keep)
            if how == "dev":
                line = re.findall(r"view: on the device: \d+ of \d+ members read, \d+ records scanned, (\d+) kept, \d+ batches, (\d+) blocks; device deflate level (\d)", r.stderr)
                assert len(line) == 1 and "device view off" not in r.stderr and int(line[0][0]) == len(keep) and line[0][2] == (level or "6"), r.stderr[-2000:]
            else:
                assert "device" not in r.stderr


@pytest.mark.parametrize("name", sorted(BAM_QUERIES))
def test_emu_view_bam_to_bam(emu_viewer, name):
    check_bam_out(emu_viewer, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BAM_QUERIES))
def test_gpu_view_bam_to_bam(gpu_viewer, name):
    check_bam_out(gpu_viewer, name)


def gzip_members(bam):
    out, o = [], 0
    while o < len(bam):
        out.append(o)
        o += struct.unpack_from("<H", bam, o + 16)[0] + 1
    return out


def check_against_samtools(v):
    """samtools 1.3.1 counts and names the same records for the filters that are flag masks with a MAPQ floor (none may be skipped: without the binary this fails)"""
    assert os.path.exists(SAMTOOLS), "oracle/_ref/samtools is not built"
    for name, (expr, args) in sorted(QUERIES.items()):
        if args is None:
            continue
        cnt = subprocess.run([SAMTOOLS, "view", "-c"] + list(args) + [v.d + "/sorted.bam"], capture_output=True, check=True).stdout
        names = [l.split(b"\t")[0] for l in subprocess.run([SAMTOOLS, "view"] + list(args) + [v.d + "/sorted.bam"], capture_output=True, check=True).stdout.split(b"\n")[:-1]]
        check_query(v, name)                                             # (its runs are kept: nothing runs twice)
        for how in ("host", "dev"):
            if expr:
                ours = v.runs["%s_%s" % (name, "sorted.bam_host" if how == "host" else "blocks.bam_dev")].stdout.split(b"\n")[:-1]
                assert [l.split(b"\t")[0] for l in ours] == names and b"%d\n" % len(names) == cnt, (name, how)
            else:
                assert v.runs["%s_sorted.bam_%s_c" % (name, how)].stdout == cnt, (name, how)


def test_emu_view_agrees_with_samtools(emu_viewer):
    check_against_samtools(emu_viewer)


@pytest.mark.gpu
def test_gpu_view_agrees_with_samtools(gpu_viewer):
    check_against_samtools(gpu_viewer)


# what turns the device view off: the file, the environment, whether the file comes through a pipe, the reason in the one log line
VIEW_FALLBACKS = {
    "skew": ("skew.bam", {}, False, r"device view off \(.*skew\.bam is not record-aligned at hint \d+"),
    "pipe": ("blocks.bam", {}, True, r"device view off \(an input is not a regular file"),
    "level0": ("blocks.bam", {}, False, r"device view off \(-l 0"),
    "pool": ("blocks.bam", {"SSG_VIEW_POOL": "30000"}, False, r"device view off \(.*capacity"),
    "nodev": ("blocks.bam", {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}, False, r"device view off \(no device"),   # (the emulation always has a device)
}


def check_view_fallback(v, name):
    bam, extra, pipe, reason = VIEW_FALLBACKS[name]
    if name in ("level0", "pool"):   # BAM out of a region: the host's file, byte for byte
        outs = []
        for how, env in (("host", {}), ("dev", dict(VIEW_DEV, **extra))):
            out = "%s/fb_%s_%s.bam" % (v.d, name, how)
            r = v.run("fb_%s_%s" % (name, how), ["-f", "bam"] + (["-l", "0"] if name == "level0" else []) + ["-o", out, bam, "ctgA:1-200000"], env)
            assert r.returncode == 0, r.stderr[-2000:]
            assert (len([l for l in r.stderr.split("\n") if re.search(reason, l)]) == 1 and "on the device" not in r.stderr) if how == "dev" else "device" not in r.stderr, r.stderr[-2000:]
            outs.append(open(out, "rb").read())
        assert outs[0] == outs[1] and ref.records(gzip.decompress(outs[0]), len(v.header))
        return
    expr = QUERIES["usual"][0]
    data = open(v.d + "/" + bam, "rb").read() if pipe else None
    for args in (["-c", "-F", expr], ["-F", expr]):
        host = v.run("fbhost_%s_%d" % (name, len(args)), args + ["/dev/stdin" if pipe else bam], {}, stdin=data)
        dev = v.run("fb_%s_%d" % (name, len(args)), args + ["/dev/stdin" if pipe else bam], dict(VIEW_DEV, **extra), stdin=data)
        assert dev.returncode == 0 and len([l for l in dev.stderr.split("\n") if re.search(reason, l)]) == 1 and "on the device" not in dev.stderr, dev.stderr[-2000:]
        assert dev.stdout == host.stdout and host.stdout == v.run("usual_sorted.bam_host" + ("_c" if "-c" in args else ""), args + ["sorted.bam"], {}).stdout


@pytest.mark.parametrize("name", ["skew", "pipe", "level0", "pool"])
def test_emu_view_fallbacks_give_the_host_bytes(emu_viewer, name):
    check_view_fallback(emu_viewer, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(VIEW_FALLBACKS))
def test_gpu_view_fallbacks_give_the_host_bytes(gpu_viewer, name):
    check_view_fallback(gpu_viewer, name)


REFUSED = [   # the filter, the words
    ("[NM] == 0", "`[NM]' is not supported by this filter"),
    ("read_name =~ /^gv/", "`read_name' is not supported by this filter"),
    ("mapping_quality =~ 3", "`=~' is not supported by this filter"),
    ("position > 100", "`position' is not supported by this filter"),
    ("mate_position > 100", "`mate_position' is not supported by this filter"),
    ("cigar == 100", "`cigar' is not supported by this filter"),
    ("sequence == 100", "`sequence' is not supported by this filter"),
    ("mapping_quality >= ref_id", "`ref_id' is not supported by this filter"),
    ("(paired and unmapped", "unbalanced parenthesis"),
    ("paired and unmapped)", "unbalanced parenthesis"),
    ("paired and", "syntax error at the end"),
    ("paired unmapped", "syntax error at `unmapped'"),
    ("mapping_quality >= 99999999999", "does not fit 32 bits"),
    (" or ".join(["paired"] * 33), "more than 64 operations"),
    ("", "an empty expression"),
]


def check_view_refusals_and_old_paths(v):
    for k, (expr, words) in enumerate(REFUSED):
        for extra in ({}, VIEW_DEV):
            r = v.run("refused_%d_%d" % (k, len(extra)), ["-c", "-F", expr, "sorted.bam"], extra)
            assert r.returncode == 1 and r.stdout == b"" and "view: filter: " in r.stderr and words in r.stderr, (expr, r.stderr)
    r = v.run("refused_sam_in", ["-S", "-c", "in.sam"], {})
    assert r.returncode == 1 and "-F, -c, -o, -L and regions are supported for a BAM file" in r.stderr
    r = v.run("refused_format", ["-f", "cram", "-F", "paired", "sorted.bam"], {})
    assert r.returncode == 1 and "-F, -c, -o, -L and regions are supported for a BAM file" in r.stderr
    # a region without an index, with a stale one, with one that is not a BAI file, with one of another file
    for k, (make, words) in enumerate(((lambda p: None, "regions need the index"), (lambda p: (open(p + ".bai", "wb").write(open(v.d + "/sorted.bam.bai", "rb").read()), os.utime(p, (2 ** 31 - 2, 2 ** 31 - 2))), "is older than"),
                                       (lambda p: open(p + ".bai", "wb").write(b"BAM\1" + bytes(40)), "wrong magic"), (lambda p: open(p + ".bai", "wb").write(b"BAI\1" + struct.pack("<i", 1 << 30)), "does not fit the file"),
                                       (lambda p: open(p + ".bai", "wb").write(open(v.d + "/sorted.bam.bai", "rb").read()[:300]), "truncated"),
                                       (lambda p: open(p + ".bai", "wb").write(b"BAI\1" + struct.pack("<iiiq", 1, 0, 0, 0)), "has 1 references, the header of"))):
        p = "%s/noidx_%d.bam" % (v.d, k)
        open(p, "wb").write(open(v.d + "/sorted.bam", "rb").read())
        make(p)
        for extra in ({}, VIEW_DEV):
            r = v.run("index_refused_%d_%d" % (k, len(extra)), ["-c", p, "ctgA:1-1000"], extra)
            assert r.returncode == 1 and r.stdout == b"" and words in r.stderr and "noidx_%d.bam.bai" % k in r.stderr, (k, r.stderr)
        assert v.run("index_unneeded_%d" % k, ["-c", p], {}).stdout == b"%d\n" % len(v.records)      # (without a region no index is asked for)
    r = v.run("refused_option", ["-s", "0.5", "sorted.bam"], {})
    assert r.returncode == 1 and "view: unsupported option -s" in r.stderr
    open(v.d + "/bad.bed", "w").write("ctgA\t10\t20\nctgX\t1\t2\n")
    open(v.d + "/worse.bed", "w").write("ctgA\t20\t10\n")
    for k, (args, words) in enumerate(((["sorted.bam", "ctgX:1-100"], "unknown contig `ctgX' in the region `ctgX:1-100'"), (["sorted.bam", "ctgA", "*"], "the region `*'"),
                                       (["sorted.bam", "ctgA:0-100"], "malformed region `ctgA:0-100'"), (["sorted.bam", "ctgA:200-100"], "malformed region"), (["sorted.bam", "ctgA:1x-100"], "malformed region"),
                                       (["-L", "bad.bed", "sorted.bam"], "unknown contig `ctgX' in line 2"), (["-L", "worse.bed", "sorted.bam"], "malformed line 1"), (["-L", "none.bed", "sorted.bam"], "cannot open"))):
        for extra in ({}, VIEW_DEV):
            r = v.run("refused_region_%d_%d" % (k, len(extra)), ["-c"] + [v.d + "/" + a if a.endswith(".bed") else a for a in args], extra)
            assert r.returncode == 1 and r.stdout == b"" and words in r.stderr, (args, r.stderr)
    # a filter that keeps everything prints the whole file's text; the invocations without new options say nothing new, with the switch or without
    assert v.run("all", ["-F", "not supplementary or supplementary", "blocks.bam"], VIEW_DEV).stdout == b"".join(l + b"\n" for l in v.lines)
    for extra in ({}, VIEW_DEV):
        r = v.run("old_whole_%d" % len(extra), ["blocks.bam"], extra)
        assert r.returncode == 0 and r.stdout == b"".join(l + b"\n" for l in v.lines) and "[sambamba] view" not in r.stderr
        r = v.run("old_H_%d" % len(extra), ["-H", "sorted.bam"], extra)
        l_text, = struct.unpack_from("<i", v.header, 4)
        assert r.returncode == 0 and r.stdout == v.header[8:8 + l_text].rstrip(b"\0") and "[sambamba] view" not in r.stderr
        r = v.run("old_S_%d" % len(extra), ["-S", "-f", "bam", "in.sam"], extra)
        assert r.returncode == 0 and r.stdout == open(v.d + "/in.u.bam", "rb").read() and r.stdout.endswith(EOF_MARKER) and "[sambamba] view" not in r.stderr
    # a -o file that a failing command began is not left behind
    out = v.d + "/partial.sam"
    bad = open(v.d + "/sorted.bam", "rb").read()
    open(v.d + "/cut.bam", "wb").write(bad[:len(bad) // 2])
    r = v.run("partial", ["-o", out, "-F", "not unmapped", "cut.bam"], {})
    assert r.returncode == 1 and not os.path.exists(out), r.stderr


def test_emu_view_refusals_and_old_invocations(emu_viewer):
    check_view_refusals_and_old_paths(emu_viewer)


@pytest.mark.gpu
def test_gpu_view_refusals_and_old_invocations(gpu_viewer):
    check_view_refusals_and_old_paths(gpu_viewer)
