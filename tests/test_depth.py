"""Coverage on the device (k_depth.h; ssg_depth_*; `sambamba depth'): the counters of a span, their sums over pairs of positions and the text of `samtools depth'
against tests/depth_reference.py -- a model that shares no code with the product: it decodes the records with struct and fills plain lists position by position --
at every wave and workgroup edge of the compaction, every CIGAR operation, the quality test, the clipping to a span, the LDS tile of the accumulating kernel
(SSG_DEPTH_TILE: its positions; 0 turns it off) and 64-bit sums; every refusal by its words; and the command against the model and against samtools 1.3.1 (depth,
bedcov).  CPU-side on the host emulation of the kernels; `-m gpu' on the MI355X."""
import functools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import depth_reference as model
import view_reference as ref
from common import ROOT
from speedseq_amd import capi
from test_bam_scan import OURS, load, make_member, reblock, rec
from test_bam_select import COUNTS, PATTERNS, group, marked
from test_bgzf_inflate import concat

SSG_EIO, SSG_EINVAL, SSG_EALIGN, SSG_EOVERFLOW = -5, -22, -71, -75
M, I, D, N, S, H, P, EQ, X = range(9)
DEFAULT = model.DEFAULT_FILTER


def quals(r, q):
    """a record of rec() with other quality bytes (as many as its l_seq)"""
    b = bytearray(r)
    l_qname, nc, l_seq = b[12], struct.unpack_from("<H", b, 16)[0], struct.unpack_from("<i", b, 20)[0]
    assert len(q) == l_seq
    o = 36 + l_qname + 4 * nc + (l_seq + 1) // 2
    b[o:o + l_seq] = bytes(q)
    return bytes(b)


def query_len(cigar):
    return sum(n for n, op in cigar if op in model.QUERY_OPS)


def qrec(tid, pos, cigar, q, flag=0, name=b"r\0"):
    """a record whose quality bytes cycle through q"""
    n = query_len(cigar)
    return quals(rec(tid, pos, flag, cigar, name=name, l_seq=n), [q[k % len(q)] for k in range(n)])


@functools.lru_cache(maxsize=None)
def reference_of(stream):
    return ref.records(stream, 0)


class Dev:
    """payloads in a store and a depth object on it; tile: SSG_DEPTH_TILE while the object is made"""

    def __init__(self, lib, payloads, expr=DEFAULT, q=0, tile=None):
        self.lib = lib
        self.recs, self.cid, self.off = load(lib, payloads)
        self.want = reference_of(b"".join(payloads))
        self.expr, self.q = expr, q
        old = os.environ.get("SSG_DEPTH_TILE")
        if tile is not None:
            os.environ["SSG_DEPTH_TILE"] = str(tile)
        try:
            rc, self.d = capi.depth_create(lib, self.recs, ref.postfix(expr) if expr else (), q)
        finally:
            if tile is not None:
                if old is None:
                    del os.environ["SSG_DEPTH_TILE"]
                else:
                    os.environ["SSG_DEPTH_TILE"] = old
        assert rc == 0, lib.l.ssg_last_error()

    def span(self, tid, beg, end, pushes=1):
        """begin, push, finish; the push's numbers and the counters are the model's.  Returns (span, cov) as lists."""
        lib = self.lib
        assert capi.depth_begin(lib, self.d, tid, beg, end) == 0, lib.l.ssg_last_error()
        for _ in range(pushes):
            rc, n_rec, n_used, n_later, desc, behind = capi.depth_push(lib, self.d, self.cid, self.off)
            assert rc == 0, lib.l.ssg_last_error()
            assert (n_rec,) + (n_used, n_later, desc, behind) == (len(self.want),) + model.push_numbers(self.want, self.expr, tid, beg, end)
        assert capi.depth_finish(lib, self.d) == 0, lib.l.ssg_last_error()
        rc, span, cov = capi.depth_get(lib, self.d, beg, end)
        assert rc == 0, lib.l.ssg_last_error()
        ws, wc = model.counters(self.want, self.expr, self.q, tid, beg, end)
        assert [int(x) // pushes for x in span] == ws and [int(x) // pushes for x in cov] == wc
        assert all(int(x) % pushes == 0 for x in span)
        return ws, wc

    def end(self):
        assert capi.depth_end(self.lib, self.d) == 0

    def span2(self, tid, beg, end):
        """the open span closed, then span()"""
        self.end()
        return self.span(tid, beg, end)

    def close(self):
        self.d.close()
        self.recs.close()


# ---- the compaction of the used records: wave and workgroup edges, six patterns ----
def check_compaction(lib, name):
    payloads = marked(name)
    for pat, expr in PATTERNS.items():
        d = Dev(lib, payloads, expr)
        n = len(d.want)
        top = max(r["end"] for r in d.want) + 3
        s, _ = d.span(1, 0, top)
        kept = ref.select(d.want, (), expr)
        assert (sum(s) > 0) == any(d.want[i]["tid"] == 1 for i in kept), pat
        assert pat != "everything" or len(kept) == n
        d.end()
        d.close()


@pytest.mark.parametrize("name", COUNTS)
def test_emu_depth_compaction_edges(emu_lib, name):
    check_compaction(emu_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", COUNTS)
def test_gpu_depth_compaction_edges(gpu_lib, name):
    check_compaction(gpu_lib, name)


# ---- the CIGAR walk ----
@functools.lru_cache(maxsize=None)
def cigar_payloads():
    recs, pos = [], 100
    def add(cigar, tid=0, flag=0):
        nonlocal pos
        recs.append(qrec(tid, pos, cigar, [30, 10, 20, 19, 21, 255], flag))
        pos += 7
    for op in range(9):                                                   # every operation first, in the middle and last, and in runs of 1
        add([(5, op), (9, M), (4, M)]); add([(6, M), (5, op), (7, M)]); add([(8, M), (3, op)]); add([(1, op), (1, M), (1, op)])
    add([(10, M), (3, D), (10, M)]); add([(10, M), (30, N), (10, M)]); add([(3, S), (2, I), (10, M), (2, I), (4, S)])
    add([(4, D), (10, M)]); add([(5, S), (5, I)]); add([(1, EQ), (1, X), (1, M)])
    recs.append(rec(0, pos, 0, [], l_seq=10)); pos += 7                    # a mapped record without CIGAR: nothing
    for n in (1, 2, 64, 65, 300):
        add([(1 + k % 3, (M, D, M, I, M, N, EQ, S, X)[k % 9] if 0 < k < n - 1 else M) for k in range(n)])
    recs.append(rec(-1, pos, 0, [(20, M)], l_seq=20))                      # tid == -1: nothing (and behind every span)
    return tuple(group(recs))


def check_cigars(lib):
    payloads = list(cigar_payloads())
    top = max(r["end"] for r in reference_of(b"".join(payloads))) + 5
    got = {}
    for q in (0, 20):
        for tile in (None, 0):
            d = Dev(lib, payloads, DEFAULT, q, tile)
            got[q, tile] = d.span(0, 0, top)
            d.end(); d.close()
        assert got[q, None] == got[q, 0]
    assert got[0, None][0] == got[20, None][0] and got[0, None][1] != got[20, None][1]   # span does not look at qualities, cov does
    # a record flagged unmapped that a filter lets pass: its end is pos + 1 (bam_endpos) for the overlap test, and its operations count where they lie
    flagged = group([rec(0, 100, 4, [(30, M)], l_seq=30), rec(0, 105, 0, [(10, M)], l_seq=10), rec(0, 300, 4, [(5, M), (10, D), (5, M)], l_seq=10)])
    for q in (0, 20):
        for tile in (64, 0):
            d = Dev(lib, flagged, "", q, tile)
            assert sum(d.span(0, 90, 400)[0]) == 60 and sum(d.span2(0, 101, 400)[0]) == 30
            d.close()
    assert max(got[0, None][0]) > 2 and 0 in got[20, None][1]


def test_emu_depth_cigar_walk(emu_lib):
    check_cigars(emu_lib)


@pytest.mark.gpu
def test_gpu_depth_cigar_walk(gpu_lib):
    check_cigars(gpu_lib)


# ---- the quality test ----
def check_qualities(lib, q):
    cyc = [max(q - 1, 0), q, min(q + 1, 255), 255, 0]
    recs, pos = [], 50
    for n in (1, 63, 64, 65, 150, 310):
        for pre in ([], [(1, S)], [(2, S), (1, I)], [(2, I)]):              # query offsets odd and even before the first M
            recs.append(qrec(0, pos, pre + [(n, M)], cyc)); pos += 3
            recs.append(qrec(0, pos, pre + [(n, M), (2, D), (5, X), (1, I), (3, EQ)], cyc[::-1])); pos += 3
    recs.append(rec(0, pos, 0, [(40, M)], l_seq=0))                          # no sequence: every base passes
    recs.append(quals(rec(0, pos + 1, 0, [(40, M)], l_seq=40), [255] * 40))  # no qualities (0xff): every base passes
    recs.append(quals(rec(0, pos + 2, 0, [(40, M)], l_seq=25), [0] * 25))    # qualities end before the CIGAR does: the bases beyond pass
    payloads = group(recs)
    top = max(r["end"] for r in reference_of(b"".join(payloads))) + 5
    for tile in (None, 0):
        d = Dev(lib, payloads, DEFAULT, q, tile)
        s, c = d.span(0, 0, top)
        assert s != c
        d.end()
        s2, c2 = d.span(0, 60, 200)                                           # clipped at both ends, the same object
        assert (s2, c2) == (s[60:200], c[60:200])
        d.end(); d.close()


@pytest.mark.parametrize("q", [1, 20, 255])
def test_emu_depth_base_quality(emu_lib, q):
    check_qualities(emu_lib, q)


@pytest.mark.gpu
@pytest.mark.parametrize("q", [1, 20, 255])
def test_gpu_depth_base_quality(gpu_lib, q):
    check_qualities(gpu_lib, q)


# ---- clipping to the span ----
def check_clipping(lib):
    beg, end = 1000, 1100
    recs = [rec(0, 1050, 0, [(20, M)]),                                       # tid lower than the span's
            rec(1, 950, 0, [(80, M)]), rec(1, 960, 0, [(40, M)]),             # starts before beg and ends inside; ends exactly at beg
            rec(1, 900, 0, [(50, M), (100, N), (50, M), (200, D), (10, M)]),  # covers the whole span and more
            rec(1, 1040, 0, [(10, M), (5, D), (10, M)]),
            rec(1, 1099, 0, [(30, M)]), rec(1, 1100, 0, [(30, M)]),           # starts at end - 1; starts at end
            rec(2, 1050, 0, [(20, M)])]                                       # tid greater than the span's
    payloads = group(recs)
    for q in (0, 20):
        d = Dev(lib, payloads, DEFAULT, q)
        s, c = d.span(1, beg, end)
        assert model.push_numbers(d.want, DEFAULT, 1, beg, end)[:2] == (4, 4)
        d.end()
        for p in (beg, 1049, end - 1):                                         # a span of one position
            assert d.span(1, p, p + 1) == ([s[p - beg]], [c[p - beg]])
            d.end()
        parts = []
        for b, e in ((900, 1000), (1000, 1033), (1033, 1300)):                 # the same chunk pushed into three consecutive spans
            parts.append(d.span(1, b, e)); d.end()
        wide = d.span(1, 900, 1300); d.end()
        assert (sum((p[0] for p in parts), []), sum((p[1] for p in parts), [])) == wide
        d.span(1, beg, end, pushes=2); d.end()                                  # integer adds: a chunk pushed twice counts twice
        d.close()


def test_emu_depth_clipping(emu_lib):
    check_clipping(emu_lib)


@pytest.mark.gpu
def test_gpu_depth_clipping(gpu_lib):
    check_clipping(gpu_lib)


# ---- the LDS tile (SSG_DEPTH_TILE positions) ----
T = 64


def check_tile(lib):
    cases = {}
    for stretch in (T - 1, T, T + 1):                                           # one workgroup whose records reach over `stretch' positions
        cases["stretch_%d" % stretch] = [qrec(0, 500 + k % (stretch - 9), [(10, M)], [30, 5]) for k in range(200)] + [qrec(0, 500 + stretch - 10, [(10, M)], [30, 5])]
    cases["crossing"] = [qrec(0, 500 + k // 8, [(20, M)], [30, 5]) for k in range(256)] + [qrec(0, 500 + 32, [(T, M)], [30, 5])] + [qrec(0, 540 + k // 8, [(20, M)], [30, 5]) for k in range(255)]
    cases["long_n"] = [qrec(0, 500 + k % 20, [(10, M)], [30, 5]) for k in range(100)] + [qrec(0, 520, [(10, M), (10 * T, N), (10, M)], [30, 5])] + [qrec(0, 521 + k % 20, [(10, M)], [30, 5]) for k in range(100)]
    cases["pile"] = [qrec(0, 500, [(30, M), (2, D), (8, M)], [30, 5]) for _ in range(300)]
    for name, recs in cases.items():
        recs = sorted(recs, key=lambda r: struct.unpack_from("<i", r, 8)[0])
        payloads = group(recs)
        for q in (0, 20):
            got = []
            for tile in (T, None, 0):
                d = Dev(lib, payloads, DEFAULT, q, tile)
                got.append(d.span(0, 490, 1300)); d.end()
                got.append(d.span(0, 510, 530)); d.end()                       # and with the span's ends inside the stretch
                d.close()
            assert got[0] == got[2] == got[4] and got[1] == got[3] == got[5], (name, q)


def test_emu_depth_tile(emu_lib):
    check_tile(emu_lib)


@pytest.mark.gpu
def test_gpu_depth_tile(gpu_lib):
    check_tile(gpu_lib)


# ---- 32-bit counters, 64-bit sums ----
def check_width(lib):
    n, ln = 5000, 1000000
    d = Dev.__new__(Dev)
    d.lib = lib
    d.recs, d.cid, d.off = load(lib, group([rec(0, 0, 0, [(ln, M)], name=b"w%d\0" % k) for k in range(n)], (64,)))
    rc, d.d = capi.depth_create(lib, d.recs, ref.postfix(DEFAULT), 0)
    assert rc == 0
    assert capi.depth_begin(lib, d.d, 0, 0, ln) == 0
    assert capi.depth_push(lib, d.d, d.cid, d.off) == (0, n, n, 0, 0, 0)
    assert capi.depth_finish(lib, d.d) == 0
    rc, span, cov = capi.depth_get(lib, d.d, 0, ln)
    assert rc == 0 and (span == n).all() and (cov == n).all()
    rc, out = capi.depth_sums(lib, d.d, [(0, ln), (7, 8)], [0, 1, 5000, 5001])
    assert rc == 0 and [[int(x) for x in row] for row in out] == [[n * ln, n * ln, ln, ln, ln, 0], [n, n, 1, 1, 1, 0]]
    assert n * ln > 1 << 32
    d.end(); d.close()


def test_emu_depth_width(emu_lib):
    check_width(emu_lib)


@pytest.mark.gpu
def test_gpu_depth_width(gpu_lib):
    check_width(gpu_lib)


# ---- sums over pairs ----
def check_sums(lib):
    rng = np.random.RandomState(5)
    beg, end = 1000, 1000 + 100003
    recs = sorted((qrec(0, int(rng.randint(900, end + 50)), [(int(rng.randint(1, 120)), M), (int(rng.randint(1, 9)), D), (int(rng.randint(1, 60)), M)], [30, 2, 40]) for _ in range(3000)),
                  key=lambda r: struct.unpack_from("<i", r, 8)[0])
    d = Dev(lib, group(recs), DEFAULT, 20)
    s, c = d.span(0, beg, end)
    thr = [0, 1, 2, 3]
    pairs = [(beg, beg + 1), (end - 1, end), (2000, 2100), (2100, 2200), (2050, 2150), (2050, 2150), (1500, 1501), (beg, end), (90000, 99000), (1200, 9000)]
    pairs += [(w, min(w + 4097, end)) for w in range(beg, end, 4097)]                                  # windows, the last one short
    for ps, th in ((pairs, thr), (pairs[:3], []), ([(p, p + 1) for p in range(beg, beg + 100000)], [1])):    # 100 000 windows of one position
        rc, out = capi.depth_sums(lib, d.d, ps, th)
        assert rc == 0, lib.l.ssg_last_error()
        assert [[int(x) for x in row] for row in out] == model.sums(beg, s, c, ps, th)
    rc, out = capi.depth_sums(lib, d.d, [], thr)                                                          # no pair
    assert rc == 0 and out.shape == (0, 6)
    for bad, words in (([(beg - 1, beg + 5)], "not inside the span"), ([(beg, end + 1)], "not inside the span"), ([(2000, 2000)], "beg >= end"), ([(2001, 2000)], "beg >= end")):
        rc, out = capi.depth_sums(lib, d.d, [(beg, end)] + bad, thr)
        assert rc == SSG_EINVAL and words in lib.l.ssg_last_error().decode() and "ssg_depth_sums: pair 1" in lib.l.ssg_last_error().decode()
        assert (out == 0xABABABABABABABAB).all()
    rc, _ = capi.depth_sums(lib, d.d, pairs[:1], list(range(9)))
    assert rc == SSG_EINVAL and "n_thr outside 0 .. 8" in lib.l.ssg_last_error().decode()
    d.end(); d.close()


def test_emu_depth_sums(emu_lib):
    check_sums(emu_lib)


@pytest.mark.gpu
def test_gpu_depth_sums(gpu_lib):
    check_sums(gpu_lib)


# ---- text ----
def check_text(lib):
    # the digits of the position: a span around every power of ten up to 10^9
    for k in range(1, 10):
        p10 = 10 ** k
        b, e = p10 - 8, p10 + 8
        d = Dev(lib, group([rec(0, max(p10 - 12, 0), 0, [(8, M)]), rec(0, p10 - 3, 0, [(2, M), (3, D), (2, M)]), rec(0, p10 + 1, 0, [(40, M)])]))
        s, c = d.span(0, b, e)
        for every in (False, True):
            rc, text, n = capi.depth_text(lib, d.d, "c", b, e, every)
            assert rc == 0 and text == model.text("c", b, s, c, b, e, every) and n == len(text)
        assert b"c\t%d\t" % (p10 - 1) in text and b"c\t%d\t" % p10 in text and b"\t0\n" in text
        d.end(); d.close()
    # the digits of cov: 9 -> 10 and 99 -> 100; names of 1 and 255 bytes; skipped positions at both ends; cuts at every offset of 70 positions
    recs = [rec(0, 120, 0, [(10, M)]) for _ in range(9)] + [rec(0, 125, 0, [(10, M)])] + [rec(0, 140, 0, [(10, M)]) for _ in range(99)] + [rec(0, 145, 0, [(3, M), (4, N), (3, M)])]
    d = Dev(lib, group(recs))
    b, e = 100, 170
    s, c = d.span(0, b, e)
    assert {9, 10, 99, 100} <= set(c) and s[0] == 0 and s[-1] == 0
    for name in ("x", "n" * 255):
        for every in (False, True):
            whole = model.text(name, b, s, c, b, e, every)
            rc, text, n = capi.depth_text(lib, d.d, name, b, e, every)
            assert rc == 0 and text == whole
            rc, text, n = capi.depth_text(lib, d.d, name, b, e, every, cap=0)                            # the sizing form
            assert rc == 0 and text == b"" and n == len(whole)
            rc, text, n = capi.depth_text(lib, d.d, name, b, e, every, cap=len(whole) - 1)                # one byte short: nothing written
            assert rc == SSG_EOVERFLOW and n == len(whole) and "bytes of text, room for" in lib.l.ssg_last_error().decode()
            if name == "x":
                for cut in range(b, e + 1):
                    assert capi.depth_text(lib, d.d, name, b, cut, every)[1] + capi.depth_text(lib, d.d, name, cut, e, every)[1] == whole
    for p0, p1, words in ((b - 1, e, "not inside the span"), (b, e + 1, "not inside the span"), (e, b, "not inside the span")):
        rc, _, _ = capi.depth_text(lib, d.d, "x", p0, p1)
        assert rc == SSG_EINVAL and words in lib.l.ssg_last_error().decode()
    assert capi.depth_text(lib, d.d, "", b, e)[0] == SSG_EINVAL
    d.end()
    s, c = d.span(0, 5000, 5040)                                                                            # a span without a record
    assert capi.depth_text(lib, d.d, "x", 5000, 5040, False)[1:] == (b"", 0)
    assert capi.depth_text(lib, d.d, "x", 5000, 5040, True)[1] == b"".join(b"x\t%d\t0\n" % (p + 1) for p in range(5000, 5040))
    d.end(); d.close()


def test_emu_depth_text(emu_lib):
    check_text(emu_lib)


@pytest.mark.gpu
def test_gpu_depth_text(gpu_lib):
    check_text(gpu_lib)


# ---- refusals and state ----
BAD_PROGRAMS = [([(capi.FOP_AND, 0, 0)], "operation 0 underflows the stack"), ([(capi.FOP_NOT, 0, 0)], "operation 0 underflows the stack"),
                ([(capi.FOP_FLAG, 0, 4), (capi.FOP_FLAG, 0, 8)], "the filter program leaves 2 values, not exactly one"),
                ([(capi.FOP_FLAG, 0, 4), (11, 0, 0)], "operation 1 is the unknown operation 11"), ([(capi.FOP_EQ, 6, 0)], "operation 0 compares the unknown field 6"),
                ([(capi.FOP_FLAG, 0, 4)] + [(capi.FOP_NOT, 0, 0)] * 64, "a filter program of 65 operations, at most 64 are taken")]


def err(lib):
    return lib.l.ssg_last_error().decode()


def check_refusals(lib):
    good = group([rec(0, 100 + 3 * k, 0, [(20, M)]) for k in range(10)])
    recs, cid, off = load(lib, good)
    for prog, words in BAD_PROGRAMS:                                            # what ssg_recs_select refuses of a program, in its words
        rc, d = capi.depth_create(lib, recs, prog, 0)
        assert rc == SSG_EINVAL and d is None and err(lib) == "ssg_depth_create: " + words
        rc2 = capi.recs_select(lib, recs, cid, off, prog=prog)[0]
        assert rc2 == SSG_EINVAL and err(lib) == "ssg_recs_select: " + words
    for q in (-1, 256):
        rc, d = capi.depth_create(lib, recs, (), q)
        assert rc == SSG_EINVAL and "min_baseq outside 0 .. 255" in err(lib)
    assert capi.depth_create(lib, None, (), 0)[0] == SSG_EINVAL
    rc, d = capi.depth_create(lib, recs, ref.postfix(DEFAULT), 0)
    assert rc == 0
    # state: nothing without a span, one span at a time, no push behind finish
    assert capi.depth_push(lib, d, cid, off)[0] == SSG_EINVAL and "no span is open" in err(lib)
    assert capi.depth_finish(lib, d) == SSG_EINVAL and capi.depth_end(lib, d) == SSG_EINVAL
    assert capi.depth_get(lib, d, 0, 1)[0] == SSG_EINVAL and "no finished span" in err(lib)
    for t, b, e in ((-1, 0, 10), (0, -1, 10), (0, 10, 10), (0, 11, 10), (0, 0, 1 << 31)):
        assert capi.depth_begin(lib, d, t, b, e) == SSG_EINVAL and "ssg_depth_begin" in err(lib)
    assert capi.depth_begin(lib, d, 0, 90, 200) == 0
    assert capi.depth_begin(lib, d, 0, 90, 200) == SSG_EINVAL and "a span is open" in err(lib)
    assert capi.depth_get(lib, d, 90, 200)[0] == SSG_EINVAL and capi.depth_sums(lib, d, [(90, 91)])[0] == SSG_EINVAL and capi.depth_text(lib, d, "x", 90, 91)[0] == SSG_EINVAL
    assert capi.depth_push(lib, d, cid, off)[:3] == (0, 10, 10)
    # the scan's refusals under this entry's name, and the counters as they were
    rc, bad_cid, bad_off, _ = capi.recs_append_bgzf(lib, recs, *concat([make_member(p, "dynamic") for p in
                                                     (rec(0, 100, 0, [(5, M)]) + struct.pack("<I", 31) + bytes(31), rec(0, 101, 0, [(5, M)]))]))
    assert rc == 0
    rc, skew_cid, skew_off, _ = capi.recs_append_bgzf(lib, recs, *concat([make_member(p, "dynamic") for p in
                                                       (rec(0, 100, 0, [(5, M)])[:-3], rec(0, 100, 0, [(5, M)])[-3:] + rec(0, 101, 0, [(5, M)]))]))
    assert rc == 0
    for args, want_rc in (((bad_cid, bad_off), SSG_EIO), ((skew_cid, skew_off), SSG_EALIGN), ((99, off), SSG_EINVAL), ((cid, off[::-1].copy()), SSG_EINVAL)):
        got = capi.depth_push(lib, d, *args)
        words = err(lib)
        assert got[0] == want_rc and words.startswith("ssg_depth_push: "), (got, words)
        rc2 = capi.recs_scan(lib, recs, *args)[0] if want_rc != SSG_EINVAL else None
        if want_rc == SSG_EINVAL:
            try:
                capi.recs_scan(lib, recs, *args)
                assert False
            except capi.SsgError:
                pass
        else:
            assert rc2 == want_rc
        assert err(lib) == "ssg_recs_scan: " + words[len("ssg_depth_push: "):]
    assert capi.depth_finish(lib, d) == 0
    assert capi.depth_finish(lib, d) == SSG_EINVAL
    assert capi.depth_push(lib, d, cid, off)[0] == SSG_EINVAL and "the span is finished" in err(lib)
    rc, span, cov = capi.depth_get(lib, d, 90, 200)
    want = model.counters(ref.records(b"".join(good)), DEFAULT, 0, 0, 90, 200)
    assert rc == 0 and ([int(x) for x in span], [int(x) for x in cov]) == want                 # the failed pushes added nothing
    for p0, p1 in ((89, 200), (90, 201), (100, 99)):
        assert capi.depth_get(lib, d, p0, p1)[0] == SSG_EINVAL and "not inside the span" in err(lib)
    assert capi.depth_end(lib, d) == 0
    d.close()
    # a malformed record on the quality path: the sequence leaves the record
    r = bytearray(rec(0, 100, 0, [(20, M)], l_seq=20)); struct.pack_into("<i", r, 20, 4000)
    recs2, cid2, off2 = load(lib, [bytes(r)])
    for q, want_rc in ((0, 0), (20, SSG_EIO)):
        rc, d = capi.depth_create(lib, recs2, (), q)
        assert rc == 0 and capi.depth_begin(lib, d, 0, 0, 200) == 0
        assert capi.depth_push(lib, d, cid2, off2)[0] == want_rc
        assert want_rc == 0 or "malformed record at offset 0" in err(lib)
        d.close()
    recs2.close()
    # a swapped pair
    swapped = [rec(0, 100, 0, [(5, M)]), rec(0, 300, 0, [(5, M)]), rec(0, 200, 16, [(5, M)]), rec(0, 200, 0, [(5, M)]), rec(1, 5, 0, [(5, M)]), rec(0, 900, 0, [(5, M)])]
    dv = Dev(lib, group(swapped))
    dv.span(0, 0, 1000)
    assert model.push_numbers(dv.want, DEFAULT, 0, 0, 1000)[2] == 2
    dv.end(); dv.close()
    recs.close()


def test_emu_depth_refusals_and_state(emu_lib):
    check_refusals(emu_lib)


@pytest.mark.gpu
def test_gpu_depth_refusals_and_state(gpu_lib):
    check_refusals(gpu_lib)


# ---------------- sambamba depth ----------------
SAMTOOLS = os.path.join(ROOT, "oracle", "_ref", "samtools")
CONTIGS = [("cA", 30000), ("cB", 12000), ("cC", 5000)]
CIGARS = ["100M", "60M2D40M", "30S70M", "50M1000N50M", "40M3I57M", "10S20M5I30M4D30M5S", "100M"]
Q1 = "mapping_quality >= 1 and " + DEFAULT


def write_input(path, seed):
    rng = np.random.RandomState(seed)
    with open(path, "w") as f:
        f.write("@HD\tVN:1.3\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CONTIGS))
        def line(i, flag, ctg, pos, mapq, cigar, qual=True):
            n = sum(int(x) for x, op in re.findall(r"(\d+)([MIS=X])", cigar))
            seq = "".join("ACGT"[b] for b in rng.randint(0, 4, size=n))
            q = "".join(chr(33 + v) for v in rng.choice([40, 37, 20, 19, 12, 2], size=n)) if qual else "*"
            f.write("d%d\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t%s\n" % (i, flag, ctg, pos, mapq, cigar, seq, q))
        for i in range(2000):
            name, ln = CONTIGS[int(rng.choice(3, p=[0.6, 0.3, 0.1]))]
            cigar = str(rng.choice(CIGARS))
            reach = sum(int(x) for x, op in re.findall(r"(\d+)([MDN=X])", cigar))
            line(i, int(rng.choice([0, 16, 99, 147, 1024, 1024 | 16, 256, 512, 2048])), name, int(rng.randint(1, ln - reach + 2)), int(rng.choice([0, 20, 60])), cigar, qual=i % 50 != 7)
        for k, (name, ln) in enumerate(CONTIGS):                                 # the first and the last base of every contig
            line(3000 + 2 * k, 0, name, 1, 60, "100M"); line(3001 + 2 * k, 16, name, ln - 99, 60, "100M")
        for i in range(50):
            line(4000 + i, 4, "*", 0, 0, "*")


class DepthFile:
    """a coordinate-sorted, indexed BAM of about 2000 records over three contigs made through the product's own view, sort and index, as the sort wrote it and in
    blocks of about 20 kB (tens of members), and every run of `depth' on them"""

    def __init__(self, sambamba, d):
        self.sambamba, self.d, self.runs = sambamba, str(d), {}
        self.clean = {k: v for k, v in os.environ.items() if k not in OURS + ("SSG_DEPTH_SPAN", "SSG_DEPTH_TILE", "SSG_PROF")}
        write_input(self.d + "/in.sam", 21)
        with open(self.d + "/in.sam", "rb") as fi, open(self.d + "/in.u.bam", "wb") as fo:
            subprocess.run([sambamba, "view", "-S", "-f", "bam", "/dev/stdin"], stdin=fi, stdout=fo, check=True, env=self.clean)
        subprocess.run([sambamba, "sort", "-t", "4", "-m", "1G", "--tmpdir=%s/tmp" % self.d, "-o", self.d + "/sorted.bam", self.d + "/in.u.bam"], check=True, capture_output=True, env=self.clean)
        bam = open(self.d + "/sorted.bam", "rb").read()
        open(self.d + "/blocks.bam", "wb").write(reblock(bam))
        open(self.d + "/skew.bam", "wb").write(reblock(bam, step=3001))
        open(self.d + "/noindex.bam", "wb").write(bam)
        open(self.d + "/unsorted.bam", "wb").write(reblock(open(self.d + "/in.u.bam", "rb").read()))   # in.u.bam with blocks that start at records: what is wrong with it is its order
        for name in ("sorted", "blocks"):
            subprocess.run([sambamba, "index", "-t", "4", "%s/%s.bam" % (self.d, name)], check=True, capture_output=True, env=self.clean)
        self.header, self.refs, self.records = ref.read_bam(self.d + "/sorted.bam")
        assert self.refs == CONTIGS and len(self.records) == 2056
        open(self.d + "/two.bed", "w").write("cA\t100\t2500\ncC\t0\t5000\ncA\t2400\t2600\ncB\t11900\t12000\ncA\t29999\t30000\n")

    def run(self, tag, args, extra=None):
        if tag not in self.runs:
            env = dict(self.clean)
            env.update(extra or {})
            r = subprocess.run([self.sambamba, "depth"] + [self.d + "/" + a if a.endswith((".bam", ".bed")) and "/" not in a else a for a in args], capture_output=True, env=env)
            r.stderr = r.stderr.decode()
            self.runs[tag] = r
        return self.runs[tag]

    def out(self, tag, args, extra=None):
        r = self.run(tag, args, extra)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout

    @functools.lru_cache(maxsize=None)
    def model(self, expr=DEFAULT, q=0):
        return model.File(self.refs, self.records, expr, q)

    def samtools(self, *args):
        r = subprocess.run([SAMTOOLS] + list(args), capture_output=True, cwd=self.d)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout


@pytest.fixture(scope="module")
def emu_depth(tmp_path_factory, emu_lib):
    return DepthFile(os.path.join(ROOT, "tests", "emu", "sambamba_emu"), tmp_path_factory.mktemp("depth_emu"))


@pytest.fixture(scope="module")
def gpu_depth(tmp_path_factory, gpu_lib):
    return DepthFile(os.path.join(ROOT, "bin", "sambamba"), tmp_path_factory.mktemp("depth_gpu"))


BED_ITEMS = [(0, 100, 2500), (2, 0, 5000), (0, 2400, 2600), (1, 11900, 12000), (0, 29999, 30000)]
TWO = [(0, 999, 3000), (1, 10999, 12000)]                                             # cA:1000-3000 cB:11000
BASE_QUERIES = {   # name -> (arguments, (filter, min_baseq), regions, every)
    "plain": ([], (DEFAULT, 0), None, False),
    "all": (["-a"], (DEFAULT, 0), None, True),
    "q20": (["-q", "20"], (DEFAULT, 20), None, False),
    "mapq1": (["-F", Q1], (Q1, 0), None, False),
    "two_regions": (["cA:1000-3000", "cB:11000"], (DEFAULT, 0), TWO, False),
    "bed": (["-L", "two.bed"], (DEFAULT, 0), BED_ITEMS, False),
}


def base_out(v, name, bam="blocks.bam", extra=None, tag=""):
    args, _, _, _ = BASE_QUERIES[name]
    opts = [a for a in args if not (":" in a and not a.startswith("-"))]
    regions = [a for a in args if a not in opts]
    return v.out("base_%s_%s%s" % (name, bam, tag), ["base"] + opts + [bam] + regions, extra)


def check_base(v, name):
    _, (expr, q), regions, every = BASE_QUERIES[name]
    got = base_out(v, name)
    assert got == v.model(expr, q).base(regions, every)
    assert len(got) > 1000


@pytest.mark.parametrize("name", sorted(BASE_QUERIES))
def test_emu_depth_base(emu_depth, name):
    check_base(emu_depth, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BASE_QUERIES))
def test_gpu_depth_base(gpu_depth, name):
    check_base(gpu_depth, name)


def yardstick_conditions(v):
    """what the input must be for samtools 1.3.1 to be a valid yardstick"""
    mapped = [r for r in v.records if r["tid"] >= 0]
    assert all((a["tid"], a["pos"]) <= (b["tid"], b["pos"]) for a, b in zip(mapped, mapped[1:]))
    unfiltered = model.File(v.refs, v.records, "", 0)
    assert max(max(s) for s, _ in unfiltered.c) <= 4000
    for r in mapped:
        ops, _ = model.cigar_and_quals(r)
        core = [op for _, op in ops if op not in (S, H)]
        assert ops and r["l_seq"] > 0 and core[0] in model.BASE_OPS and core[-1] in model.BASE_OPS
    for t, b, e in TWO:
        assert any(model.passing(r, DEFAULT) and r["tid"] == t and r["pos"] < e and r["end"] > b for r in v.records)


def check_samtools(v):
    assert os.path.exists(SAMTOOLS)
    yardstick_conditions(v)
    assert base_out(v, "plain") == v.samtools("depth", "blocks.bam")
    assert base_out(v, "all") == v.samtools("depth", "-aa", "blocks.bam")
    assert base_out(v, "q20") == v.samtools("depth", "-q", "20", "blocks.bam")
    assert base_out(v, "mapq1") == v.samtools("depth", "-Q", "1", "blocks.bam")
    assert base_out(v, "two_regions") == v.samtools("depth", "-r", "cA:1000-3000", "blocks.bam") + v.samtools("depth", "-r", "cB:11000", "blocks.bam")
    assert base_out(v, "bed") == v.samtools("depth", "-b", "two.bed", "blocks.bam")
    four = lambda text: b"".join(b"\t".join(l.split(b"\t")[:4]) + b"\n" for l in text.split(b"\n")[:-1])
    assert four(v.out("region_bed", ["region", "-T", "1", "-T", "30", "-L", "two.bed", "blocks.bam"])) == v.samtools("bedcov", "two.bed", "blocks.bam")
    assert four(v.out("region_bed_q1", ["region", "-F", Q1, "-L", "two.bed", "blocks.bam"])) == v.samtools("bedcov", "-Q", "1", "two.bed", "blocks.bam")


def test_emu_depth_agrees_with_samtools(emu_depth):
    check_samtools(emu_depth)


@pytest.mark.gpu
def test_gpu_depth_agrees_with_samtools(gpu_depth):
    check_samtools(gpu_depth)


def check_windows_and_regions(v):
    m = v.model()
    assert v.out("window_1000", ["window", "-w", "1000", "blocks.bam"]) == m.lines(m.windows(1000))
    assert v.out("window_700_regions", ["window", "-w", "700", "-T", "2", "blocks.bam", "cA:1000-3000", "cB:11000"]) == m.lines(m.windows(700, TWO), [2])
    got = v.out("region_bed", ["region", "-T", "1", "-T", "30", "-L", "two.bed", "blocks.bam"])
    assert got == m.lines(BED_ITEMS, [1, 30])
    for l, (t, b, e) in zip(got.decode().split("\n"), BED_ITEMS):                   # lines in the BED file's order, the mean as covSum / length
        c = l.split("\t")
        assert c[:3] == [CONTIGS[t][0], str(b), str(e)] and c[5] == "%.4f" % (int(c[4]) / (e - b)) and len(c) == 8
    assert v.out("region_bed_q1", ["region", "-F", Q1, "-L", "two.bed", "blocks.bam"]) == v.model(Q1, 0).lines(BED_ITEMS)


def test_emu_depth_windows_and_regions(emu_depth):
    check_windows_and_regions(emu_depth)


@pytest.mark.gpu
def test_gpu_depth_windows_and_regions(gpu_depth):
    check_windows_and_regions(gpu_depth)


def check_spans_and_blocks(v):
    """the output does not depend on the span size or on how the file is cut into chunks"""
    for name in ("plain", "bed"):
        want = base_out(v, name)
        assert base_out(v, name, "sorted.bam") == want
        for span in ("4096", "257"):
            assert base_out(v, name, extra={"SSG_DEPTH_SPAN": span}, tag="_" + span) == want
    want = v.out("window_1000", ["window", "-w", "1000", "blocks.bam"])
    assert v.out("window_1000_sorted", ["window", "-w", "1000", "sorted.bam"]) == want
    for span in ("4096", "257"):
        assert v.out("window_1000_" + span, ["window", "-w", "1000", "blocks.bam"], {"SSG_DEPTH_SPAN": span}) == want
    assert v.out("base_tile_off", ["base", "-q", "20", "blocks.bam"], {"SSG_DEPTH_TILE": "0"}) == base_out(v, "q20")


def test_emu_depth_spans_and_blocks(emu_depth):
    check_spans_and_blocks(emu_depth)


@pytest.mark.gpu
def test_gpu_depth_spans_and_blocks(gpu_depth):
    check_spans_and_blocks(gpu_depth)


REFUSED = {   # name -> (arguments, words)
    "skew": (["base", "skew.bam"], "skew.bam is not record-aligned at hint"),
    "unsorted": (["base", "unsorted.bam"], "is not sorted by coordinate"),
    "no_index": (["base", "noindex.bam", "cA:1-100"], "regions need the index"),
    "unknown_option": (["base", "-z", "blocks.bam"], "unsupported option -z"),
    "window_without_w": (["window", "blocks.bam"], "-w SIZE is required"),
    "region_without_L": (["region", "blocks.bam"], "-L BED is required"),
}


def check_refused(v):
    for name, (args, words) in REFUSED.items():
        r = v.run("refused_" + name, args)
        assert r.returncode == 1 and r.stdout == b"" and words in r.stderr and len(r.stderr.strip().split("\n")) == 1, (name, r.returncode, r.stderr[-2000:])


def test_emu_depth_refused(emu_depth):
    check_refused(emu_depth)


@pytest.mark.gpu
def test_gpu_depth_refused(gpu_depth):
    check_refused(gpu_depth)
