"""A model of `sambamba depth' and of ssg_depth_* that shares no code with the product or its kernels: records are decoded with struct, the filter is
view_reference's (a translation of the expression to Python), the two counters are plain lists filled position by position from the definitions of
include/ssgpu.h, and text is formatted with %."""
import struct

import view_reference as ref

DEFAULT_FILTER = "not (unmapped or secondary_alignment or failed_quality_control or duplicate)"
BASE_OPS, REF_OPS, QUERY_OPS = (0, 7, 8), (0, 2, 3, 7, 8), (0, 1, 4, 7, 8)   # M = X; M D N = X; M I S = X


def cigar_and_quals(r):
    """the (length, operation) pairs and the quality bytes of a record of view_reference.records"""
    b = r["bytes"]
    l_qname, nc = b[12], struct.unpack_from("<H", b, 16)[0]
    ops = [(v >> 4, v & 0xf) for v in struct.unpack_from("<%dI" % nc, b, 36 + l_qname)]
    l_seq = r["l_seq"]
    q0 = 36 + l_qname + 4 * nc + (l_seq + 1) // 2
    return ops, b[q0:q0 + l_seq]


def passing(r, expr):
    return ref.passes(expr, r) and r["tid"] >= 0 and struct.unpack_from("<H", r["bytes"], 16)[0] > 0


def positions(r, min_baseq):
    """(reference position, counts in cov) of every position the record adds to span"""
    ops, quals = cigar_and_quals(r)
    p, q = r["pos"], 0
    for n, op in ops:
        if op in REF_OPS:
            for t in range(n):
                good = op in BASE_OPS and (q + t >= len(quals) or quals[q + t] >= min_baseq)
                yield p + t, good
            p += n
        if op in QUERY_OPS:
            q += n


def counters(recs, expr, min_baseq, tid, beg, end):
    """span[] and cov[] of the positions [beg, end) of contig tid"""
    span, cov = [0] * (end - beg), [0] * (end - beg)
    for r in recs:
        if not passing(r, expr) or r["tid"] != tid or r["pos"] >= end or r["end"] <= beg:
            continue
        for p, good in positions(r, min_baseq):
            if beg <= p < end:
                span[p - beg] += 1
                cov[p - beg] += 1 if good else 0
    return span, cov


def push_numbers(recs, expr, tid, beg, end):
    """n_used, n_later, descents, n_behind of a push of these records into the span"""
    ok = [r for r in recs if passing(r, expr)]
    used = sum(1 for r in ok if r["tid"] == tid and r["pos"] < end and r["end"] > beg)
    later = sum(1 for r in ok if r["tid"] > tid or (r["tid"] == tid and r["end"] > end))
    key = [((r["tid"] & 0xffffffff) << 32) | ((r["pos"] + 1) & 0x7fffffff) for r in recs]
    desc = sum(1 for a, b in zip(key, key[1:]) if b < a)
    behind = sum(1 for r in recs if r["tid"] < 0 or r["tid"] > tid or (r["tid"] == tid and r["pos"] >= end))
    return used, later, desc, behind


def text(name, beg, span, cov, p0, p1, every):
    """the lines of positions [p0, p1); span / cov are lists whose entry 0 is position beg"""
    return "".join("%s\t%d\t%d\n" % (name, p + 1, cov[p - beg]) for p in range(p0, p1) if every or span[p - beg] > 0).encode()


def sums(beg, span, cov, pairs, thr):
    return [[sum(span[b - beg:e - beg]), sum(cov[b - beg:e - beg])] + [sum(1 for c in cov[b - beg:e - beg] if c >= t) for t in thr] for b, e in pairs]


def merged(regions):
    out = []
    for t, b, e in sorted(regions):
        if out and out[-1][0] == t and b <= out[-1][2]:
            out[-1][2] = max(out[-1][2], e)
        else:
            out.append([t, b, e])
    return [tuple(x) for x in out]


class File:
    """the counters of every contig of a BAM file (refs, records of view_reference.read_bam) under one filter and quality floor"""

    def __init__(self, refs, records, expr=DEFAULT_FILTER, min_baseq=0):
        self.refs = refs
        self.c = [counters(records, expr, min_baseq, t, 0, ln) for t, (_, ln) in enumerate(refs)]

    def base(self, regions=None, every=False):
        """`depth base': regions as (tid, beg, end) or None for the whole file"""
        regions = [(t, 0, ln) for t, (_, ln) in enumerate(self.refs)] if regions is None else merged(regions)
        out = b""
        for t, b, e in regions:
            e = min(e, self.refs[t][1])
            if b < e:
                out += text(self.refs[t][0], 0, self.c[t][0], self.c[t][1], b, e, every)
        return out

    def lines(self, items, thr=()):
        """`depth region' / `depth window': items as (tid, beg, end)"""
        out = ""
        for t, b, e in items:
            s = sums(0, self.c[t][0], self.c[t][1], [(b, min(e, self.refs[t][1]))], thr)[0]
            out += "%s\t%d\t%d\t%d\t%d\t%s%s\n" % (self.refs[t][0], b, e, s[0], s[1], "%.4f" % (s[1] / (e - b)), "".join("\t%d" % x for x in s[2:]))
        return out.encode()

    def windows(self, size, regions=None):
        regions = [(t, 0, ln) for t, (_, ln) in enumerate(self.refs)] if regions is None else merged(regions)
        return [(t, w, min(w + size, min(e, self.refs[t][1]))) for t, b, e in regions for w in range(b, min(e, self.refs[t][1]), size)]
