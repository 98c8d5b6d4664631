"""The reference of tests/test_bam_select.py: what a region and a filter select of a stream of BAM records.  It shares no code with the product: records
are decoded with struct (a BAM file with gzip), a filter expression is evaluated by translating its tokens to a Python expression over a dict of the record's
fields, and overlap is tested by its definition: the same tid, pos < reg.end and rec.end > reg.beg, rec.end as bam_endpos gives it."""
import gzip
import re
import struct

REF_CONSUMING = (0, 2, 3, 7, 8)   # M D N = X
M64 = (1 << 64) - 1
FLAGS = {"paired": 0x1, "proper_pair": 0x2, "unmapped": 0x4, "mate_is_unmapped": 0x8, "reverse_strand": 0x10, "mate_is_reverse_strand": 0x20, "first_of_pair": 0x40,
         "second_of_pair": 0x80, "secondary_alignment": 0x100, "failed_quality_control": 0x200, "duplicate": 0x400, "supplementary": 0x800}
FIELDS = {"mapping_quality": "mapq", "ref_id": "tid", "mate_ref_id": "mtid", "template_length": "isize", "sequence_length": "l_seq", "flag": "flag"}
CMPS = ("==", "!=", "<=", ">=", "<", ">")
TOKEN = re.compile(r"\s*(==|!=|<=|>=|<|>|\(|\)|-?\d+|[A-Za-z_]+)")


def records(stream, first=0):
    """every record of stream[first:] as a dict of its fields; `off' is the offset of its block_size word"""
    out, o = [], first
    while o < len(stream):
        bs, tid, pos, bmn, fnc, l_seq, mtid, mpos, isize = struct.unpack_from("<IiiIIiiii", stream, o)
        assert bs >= 32 and o + 4 + bs <= len(stream)
        l_qname, flag, nc = bmn & 0xff, fnc >> 16, fnc & 0xffff
        end = pos + 1
        if not (flag & 4) and nc:
            end = pos + sum(v >> 4 for v in struct.unpack_from("<%dI" % nc, stream, o + 36 + l_qname) if (v & 0xf) in REF_CONSUMING)
        out.append({"off": o, "len": 4 + bs, "tid": tid, "pos": pos, "end": end, "mapq": bmn >> 8 & 0xff, "flag": flag, "l_seq": l_seq, "mtid": mtid, "mpos": mpos,
                    "isize": isize, "name": stream[o + 36:o + 36 + l_qname - 1], "bytes": stream[o:o + 4 + bs]})
        o += 4 + bs
    return out


def read_bam(path):
    """(the header's bytes up to the first record, the contigs as (name, length), the records) of a BAM file"""
    data = gzip.decompress(open(path, "rb").read())
    assert data[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", data, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, o)
    o += 4
    refs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, o)
        refs.append((data[o + 4:o + 4 + l_name - 1].decode(), struct.unpack_from("<i", data, o + 4 + l_name)[0]))
        o += 8 + l_name
    return data[:o], refs, records(data, o)


def tokens(expr):
    out, o = [], 0
    expr = expr.rstrip()
    while o < len(expr):
        m = TOKEN.match(expr, o)
        assert m, (expr, o)
        out.append(m.group(1))
        o = m.end()
    return out


def passes(expr, r):
    """the filter by translation: a flag name becomes a bit test, a field the dict's entry; and, or, not, the comparisons and the parentheses are Python's"""
    if not expr:
        return True
    py = []
    for t in tokens(expr):
        if t in FLAGS:
            py.append("((r['flag'] & %d) != 0)" % FLAGS[t])
        elif t in FIELDS:
            py.append("r['%s']" % FIELDS[t])
        else:
            assert t in CMPS or t in ("and", "or", "not", "(", ")") or re.fullmatch(r"-?\d+", t), t
            py.append(t)
    return bool(eval(" ".join(py), {"r": r}))


def overlaps(r, regions):
    """regions: (tid, beg, end), 0-based half-open, in any order; none at all is no test"""
    if not regions:
        return True
    return r["tid"] >= 0 and any(r["tid"] == t and r["pos"] < e and r["end"] > b for t, b, e in regions)


def select(recs, regions=(), expr=""):
    """the indices of the kept records, in stream order"""
    return [i for i, r in enumerate(recs) if overlaps(r, regions) and passes(expr, r)]


def loc_key_ent(r, chunk):
    """what ssg_recs_scan returns of a record: the location, the coordinate key of the sort, the entry's six fields"""
    key = ((r["tid"] << 32) & M64) | (((r["pos"] + 1) << 1) & 0xffffffff) | (1 if r["flag"] & 0x10 else 0)
    return chunk << 40 | r["off"], key, (r["tid"], r["pos"], r["end"], r["flag"], r["len"], 0)


def postfix(expr):
    """the expression as the postfix program of ssg_recs_select, (op, arg, value) triples, by precedence climbing: or < and < not < comparison.  Operation and
    field numbers as include/ssgpu.h gives them."""
    ops = {"and": 1, "or": 2, "not": 3, "==": 4, "!=": 5, "<": 6, "<=": 7, ">": 8, ">=": 9}
    fld = {"mapping_quality": 0, "ref_id": 1, "mate_ref_id": 2, "template_length": 3, "sequence_length": 4, "flag": 5}
    tk, out = tokens(expr), []
    at = [0]

    def peek():
        return tk[at[0]] if at[0] < len(tk) else None

    def take():
        at[0] += 1
        return tk[at[0] - 1]

    def primary():
        t = take()
        if t == "(":
            either()
            assert take() == ")"
        elif t == "not":
            primary()
            out.append((ops["not"], 0, 0))
        elif t in FLAGS:
            out.append((0, 0, FLAGS[t]))
        else:
            c, v = take(), int(take())
            out.append((ops[c], fld[t], v))

    def both():
        primary()
        while peek() == "and":
            take()
            primary()
            out.append((ops["and"], 0, 0))

    def either():
        both()
        while peek() == "or":
            take()
            both()
            out.append((ops["or"], 0, 0))
    either()
    assert at[0] == len(tk), expr
    return out
