"""The QC tables of `samtools stats' on the device (k_stats.h; ssg_stats_*; `sambamba stats'): every scalar and table against tests/stats_reference.py -- a model
that shares no code with the product: it decodes the records with struct, counts in plain dicts, takes its checksums from zlib.crc32 and its coverage from
intervals -- at every wave and workgroup edge, every cycle tile and nibble edge of the per-base kernel (SSG_STATS_TILE, SSG_STATS_SLAB), the GC ranges, the
insert-size orientations, the CIGAR walk of count_indels, the aux walk for NM, the checksums' byte ranges, the sliding coverage window (span, pushes in blocks),
order, and every refusal by its code and words; and the command, line by line, against samtools 1.3.1.  CPU-side on the host emulation of the kernels;
`-m gpu' on the MI355X."""
import functools
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import stats_reference as model
import view_reference as ref
from common import ROOT
from speedseq_amd import capi
from test_bam_scan import OURS, make_member, reblock, rec
from test_bam_select import COUNTS, PATTERNS, group, marked
from test_bgzf_inflate import concat

SSG_EIO, SSG_EINVAL, SSG_ERANGE, SSG_EALIGN = -5, -22, -34, -71
M, I, D, N, S, H, P, EQ, X = range(9)
INT32_MIN = -(1 << 31)
KNOBS = ("SSG_STATS_TILE", "SSG_STATS_SLAB")


def srec(tid=0, pos=0, flag=0, cigar=(), seq=(), qual=None, name=b"r\0", extra=b"", mapq=30, mtid=-1, mpos=-1, isize=0):
    """a record of rec() with these 4-bit base codes, quality bytes (30 without any), MAPQ and mate fields"""
    n = len(seq)
    b = bytearray(rec(tid, pos, flag, cigar, name=name, l_seq=n, extra=extra))
    b[13] = mapq
    struct.pack_into("<iii", b, 24, mtid, mpos, isize)
    o = 36 + len(name) + 4 * len(cigar)
    for k in range(n):
        b[o + k // 2] |= (seq[k] & 15) << (0 if k & 1 else 4)
    if qual is not None:
        assert len(qual) == n
        b[o + (n + 1) // 2:o + (n + 1) // 2 + n] = bytes(qual)
    return bytes(b)


def bases(n, k=0):
    """n base codes that run through A, C, G, T and now and then N"""
    return [(1, 2, 4, 8, 15)[(k + i + i // 7) % 5] if (k + i) % 11 else 15 for i in range(n)]


def err(lib):
    return lib.l.ssg_last_error().decode()


class Knobs:
    """SSG_STATS_TILE / SSG_STATS_SLAB while an object is made"""

    def __init__(self, tile=None, slab=None):
        self.want = {"SSG_STATS_TILE": tile, "SSG_STATS_SLAB": slab}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in KNOBS}
        for k, v in self.want.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def load_chunks(lib, chunks):
    """a store with one chunk per list of payloads; returns (store, [(chunk id, member offsets)])"""
    recs, ids = capi.recs_create(lib, 1 << 40), []
    for payloads in chunks:
        blob, moff = concat([make_member(p, ("stored", "fixed", "dynamic")[k % 3]) for k, p in enumerate(payloads)])
        rc, cid, off, st = capi.recs_append_bgzf(lib, recs, blob, moff)
        assert rc == 0 and (st == 0).all(), err(lib)
        ids.append((cid, off))
    return recs, ids


def run(lib, chunks, expr="", tile=None, slab=None, **opt):
    """the chunks pushed in order into a fresh object; (result of ssg_stats_get behind ssg_stats_finish, descents of every push)"""
    recs, ids = load_chunks(lib, chunks)
    with Knobs(tile, slab):
        rc, s = capi.stats_create(lib, recs, ref.postfix(expr) if expr else (), capi.stats_opt(**opt))
    assert rc == 0, err(lib)
    desc, n = [], 0
    for cid, off in ids:
        rc, n_rec, d = capi.stats_push(lib, s, cid, off)
        assert rc == 0, err(lib)
        desc.append(d)
        n += n_rec
    assert capi.stats_finish(lib, s) == 0, err(lib)
    rc, got = capi.stats_get(lib, s)
    assert rc == 0, err(lib)
    s.close(); recs.close()
    got["n_rec"] = n
    return got, desc


@functools.lru_cache(maxsize=None)
def modelled(stream, expr, opt):
    return model.compute(ref.records(stream, 0), expr, **{k: v for k, v in opt if k != "span"})


def check(lib, chunks, expr="", tile=None, slab=None, **opt):
    """run(), and every scalar and table is the model's; returns the result"""
    if chunks and isinstance(chunks[0], bytes):
        chunks = [chunks]
    got, desc = run(lib, chunks, expr, tile, slab, **opt)
    want = modelled(b"".join(p for c in chunks for p in c), expr, tuple(sorted(opt.items())))
    assert model.differences(got, want) == [], {k: (got[k], want[k]) for k in model.differences(got, want) if k in model.SCALARS}
    assert got["n_rec"] == sum(len(ref.records(p, 0)) for c in chunks for p in c)
    assert (sum(desc) > 0) == (want["sorted"] == 0)
    return got


# ---- wave and workgroup edges of the deciding kernel, six filter patterns ----
def check_edges(lib, name):
    payloads = marked(name)
    for pat, expr in PATTERNS.items():
        got = check(lib, payloads, expr, max_len=64)
        n = got["n_rec"]
        assert got["filtered"] == n - len(ref.select(ref.records(b"".join(payloads), 0), (), expr)), pat
    assert check(lib, [], "", max_len=64)["n_rec"] == 0 if name == "1" else True


@pytest.mark.parametrize("name", COUNTS)
def test_emu_stats_wave_and_workgroup_edges(emu_lib, name):
    check_edges(emu_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", COUNTS)
def test_gpu_stats_wave_and_workgroup_edges(gpu_lib, name):
    check_edges(gpu_lib, name)


# ---- the per-base kernel: cycle tiles, nibbles, qualities, fragments ----
LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 199, 200, 299, 300, 301, 1024)
QUALS = (0, 1, 63, 64, 254, 255)


@functools.lru_cache(maxsize=None)
def base_payloads():
    recs, pos = [], 10
    for n in LENGTHS:
        for flag in (0x40, 0x80, 0, 0x40 | 0x10, 0x80 | 0x10, 0x10, 0xc0):          # both fragments and neither, forward and reverse
            recs.append(srec(0, pos, flag, [(n, M)], [(k + n) % 16 for k in range(n)], [QUALS[(k * 5 + n) % 6] for k in range(n)]))
            pos += 3
        recs.append(srec(0, pos, 0x80 | 0x10, [(n, M)], bases(n), [255] * n)); pos += 3   # the qualities of `*'
    recs.append(srec(0, pos, 4 | 0x40, [], bases(77, 3), [40] * 77))                 # unmapped: its bases count
    recs.append(srec(0, pos, 0x100, [(50, M)], bases(50), [9] * 50))                 # secondary: nothing
    recs.append(srec(0, pos, 0x800 | 0x40, [(50, M)], bases(50), [9] * 50))          # supplementary: no bases, but covered
    return tuple(group(recs))


def check_bases(lib):
    payloads = list(base_payloads())
    want = check(lib, payloads)
    assert want["max_qual"] == 255 and want["max_len"] == 1024 and want["bases"][:, 5].sum() > 0 and want["quals"][1, 1023].sum() > 0 and want["sorted"] == 1
    for tile, slab in ((1, 1), (7, 3), (31, 5), (32, 1000000)):
        got, _ = run(lib, [payloads], tile=tile, slab=slab)
        assert model.differences(got, want) == [], (tile, slab)


def test_emu_stats_cycle_tiles_and_nibbles(emu_lib):
    check_bases(emu_lib)


@pytest.mark.gpu
def test_gpu_stats_cycle_tiles_and_nibbles(gpu_lib):
    check_bases(gpu_lib)


# ---- GC ranges ----
def check_gc(lib):
    recs = []
    for n in (1, 2, 3, 7, 100, 198, 199, 200, 201, 398, 400, 1000):
        for g in sorted({0, 1, n // 3, n // 2, n - 1, n}):
            if 0 <= g <= n:
                recs.append(srec(0, 5, 0x80 if (n + g) % 2 else 0x40, [(n, M)], [(2, 4)[k % 2] for k in range(g)] + [(1, 8, 15, 3)[k % 4] for k in range(n - g)]))
    got = check(lib, group(recs))
    empty = [(n, g) for n in (398, 400, 1000) for g in (0, 1, n // 3) if (g + 1) * 199 // n == g * 199 // n]
    assert empty and got["gc"].sum() > 0 and got["gc"][:, 198].sum() > 0


def test_emu_stats_gc_ranges(emu_lib):
    check_gc(emu_lib)


@pytest.mark.gpu
def test_gpu_stats_gc_ranges(gpu_lib):
    check_gc(gpu_lib)


# ---- insert sizes ----
@functools.lru_cache(maxsize=None)
def isize_payloads():
    recs = []
    def add(flag, pos, mpos, isize, mtid=0):
        recs.append(srec(0, pos, 1 | flag, [(20, M)], bases(20), mtid=mtid, mpos=mpos, isize=isize))
    for read1 in (0x40, 0x80):
        for rev in (0, 0x10):
            for mrev in (0, 0x20):
                for mpos in (400, 600, 500):                                  # the mate before, behind, and on the record's position
                    add(read1 | rev | mrev, 500, mpos, 300 if mpos >= 500 else -300)
    for v in (0, 1, -1, 7998, 7999, 8000, -8000, 499, 500, INT32_MIN, (1 << 31) - 1):
        add(0x40 | 0x20, 100, 700, v); add(0x80 | 0x10, 700, 100, v)
    add(0x40 | 0x20, 100, 700, 0, mtid=1); add(0x40 | 0x20, 100, 700, 5, mtid=1)       # another contig: isize 0 is not counted, any other is
    add(0x40 | 0x20 | 8, 100, 700, 300); add(0x40 | 0x20 | 4, 100, 700, 300)           # a mate or the record unmapped: no insert size
    recs.append(srec(0, 100, 0x40 | 0x20, [(20, M)], bases(20), mtid=0, mpos=700, isize=300))   # not paired
    add(0x40 | 0x20, 100, 900, 777); add(0x80 | 0x10 | 0x200, 900, 100, -777)            # a pair whose second mate a filter takes: 1 // 2 == 0
    return tuple(group(recs))


def check_isize(lib):
    payloads = list(isize_payloads())
    got = check(lib, payloads)
    assert got["isize"][:, 300].tolist() == [2, 2, 6] and got["isize"][0, 7999] > 0 and got["isize"][0, 777] == 1
    assert check(lib, payloads, "not failed_quality_control")["isize"][:, 777].sum() == 0
    small = check(lib, payloads, n_isize=500)
    assert small["isize"].shape == (3, 500) and small["isize"][0, 499] > got["isize"][0, 499]


def test_emu_stats_insert_sizes(emu_lib):
    check_isize(emu_lib)


@pytest.mark.gpu
def test_gpu_stats_insert_sizes(gpu_lib):
    check_isize(gpu_lib)


# ---- count_indels ----
def check_indels(lib):
    recs, pos = [], 50
    def add(cigar, flag=0):
        nonlocal pos
        n = sum(k for k, op in cigar if op in (M, I, S, EQ, X))
        recs.append(srec(0, pos, flag, cigar, bases(n)))
        pos += 2
    for flag in (0x40, 0x80, 0x40 | 0x10, 0x80 | 0x10, 0, 0x10):
        for op in (I, D):
            add([(3, op), (20, M)], flag); add([(20, M), (3, op)], flag); add([(9, M), (2, op), (11, M)], flag); add([(9, M), (0, op), (11, M)], flag)
        add([(5, M), (7, N), (2, H), (3, P), (5, M), (1, I), (4, M), (2, D), (3, M)], flag)       # N, H and P do not advance the cycle
        add([(2, S), (3, EQ), (4, X), (1, I), (5, M), (1, D), (2, S)], flag)                       # S, = and X do
        add([(2, H), (10, M), (300, I), (10, M), (300, D), (5, M)], flag); add([(10, M), (301, I), (10, M), (301, D), (5, M), (3, H)], flag)
    got = check(lib, group(recs))
    assert got["id"][0, 299] == 6 and got["id"][1, 299] == 6 and got["id"].sum() < got["ic"].sum() and got["max_len"] == 329
    assert got["ic"][2].sum() > 0 and got["ic"][3].sum() > 0 and got["bases_cigar"] > 0


def test_emu_stats_indels(emu_lib):
    check_indels(emu_lib)


@pytest.mark.gpu
def test_gpu_stats_indels(gpu_lib):
    check_indels(gpu_lib)


# ---- NM ----
def tag(name, ty, payload):
    return name + ty + payload


def check_nm(lib):
    other = (tag(b"XA", b"A", b"q") + tag(b"Xc", b"c", b"\xff") + tag(b"XC", b"C", b"\x07") + tag(b"Xs", b"s", b"\x01\x80") + tag(b"XS", b"S", b"\xff\xff") + tag(b"Xi", b"i", struct.pack("<i", -9))
             + tag(b"XI", b"I", struct.pack("<I", 9)) + tag(b"Xf", b"f", struct.pack("<f", 1.5)) + tag(b"XZ", b"Z", b"NMC\x05text\0") + tag(b"XH", b"H", b"4E4D\0")
             + b"".join(tag(b"B" + t, b"B", t + struct.pack("<I", 3) + bytes(3 * w)) for t, w in ((b"c", 1), (b"C", 1), (b"s", 2), (b"S", 2), (b"i", 4), (b"I", 4), (b"f", 4))))
    values = [tag(b"NM", b"c", b"\xfb"), tag(b"NM", b"C", b"\xfb"), tag(b"NM", b"s", struct.pack("<h", -300)), tag(b"NM", b"S", struct.pack("<H", 65000)),
              tag(b"NM", b"i", struct.pack("<i", -1)), tag(b"NM", b"I", struct.pack("<I", 70000)), tag(b"NM", b"I", struct.pack("<I", 0xfffffffe)),
              tag(b"NM", b"A", b"7"), tag(b"NM", b"f", struct.pack("<f", 3.0)), tag(b"NM", b"Z", b"12\0")]
    recs = []
    for k, v in enumerate(values):
        recs.append(srec(0, 10 + k, 0, [(10, M)], bases(10), extra=v))
        recs.append(srec(0, 10 + k, 0, [(10, M)], bases(10), extra=other + v + tag(b"NM", b"C", b"\x63")))       # behind every other type, and a second NM
    recs.append(srec(0, 30, 0, [(10, M)], bases(10)))                                                          # absent
    recs.append(srec(0, 30, 0, [(10, M)], bases(10), extra=other))
    recs.append(srec(0, 30, 4, [(10, M)], bases(10), extra=values[3]))                                         # unmapped: not read
    recs.append(srec(0, 30, 0, [(10, M)], bases(10), extra=tag(b"XZ", b"Z", b"no end") + values[3]))           # a Z without NUL, a d, a value cut short: the walk ends
    recs.append(srec(0, 30, 0, [(10, M)], bases(10), extra=tag(b"Xd", b"d", bytes(8)) + values[3]))
    recs.append(srec(0, 30, 0, [(10, M)], bases(10), extra=b"NMi\x01\x02"))
    recs.append(srec(0, 30, 0, [(10, M)], bases(10), extra=b"NM"))
    alone = check(lib, group(recs[:2]))
    assert alone["mismatches"] == (1 << 64) - 10
    got = check(lib, group(recs))
    assert got["mismatches"] == (2 * (-5 + 251 - 300 + 65000 - 1 + 70000 - 2)) & ((1 << 64) - 1)


def test_emu_stats_nm(emu_lib):
    check_nm(emu_lib)


@pytest.mark.gpu
def test_gpu_stats_nm(gpu_lib):
    check_nm(gpu_lib)


# ---- checksums ----
def check_checksums(lib):
    recs = []
    for name in (b"\0", b"a\0", b"n" * 254 + b"\0", b"ab\0cd\0", b"x" * 255):        # l_qname 1 and 255, a NUL inside, none at all
        for n in (0, 1, 2, 3, 4, 5, 8, 9, 150, 151):
            recs.append(srec(-1, -1, 4, [], bases(n, len(name)), [(7 * k + n) % 94 for k in range(n)], name=name))
    recs.append(srec(0, 5, 0x100, [(9, M)], bases(9), name=b"secondary\0"))          # a secondary record's bytes count
    got = check(lib, group(recs))
    assert got["chk_names"] and got["chk_reads"] and got["chk_quals"] and got["chk_reads"] != got["chk_quals"]
    filtered = check(lib, group(recs), "secondary_alignment")
    assert (filtered["chk_names"], filtered["filtered"]) == (zlib.crc32(b"secondary"), len(recs) - 1)


def test_emu_stats_checksums(emu_lib):
    check_checksums(emu_lib)


@pytest.mark.gpu
def test_gpu_stats_checksums(gpu_lib):
    check_checksums(gpu_lib)


# ---- coverage ----
@functools.lru_cache(maxsize=None)
def coverage_records():
    recs = []
    def add(tid, pos, n, flag=0):
        recs.append(srec(tid, pos, flag, [(n, M)], bases(n, pos)))
    for k in range(40):
        add(0, 1000 + 13 * k, 100 + k % 50)                                  # a contiguous stretch over many windows of 257
    add(0, 1000 + 256, 1); add(0, 1000 + 256, 300); add(0, 1000 + 257, 300)      # on a window's last position, across it, on the next one's first
    recs.sort(key=lambda r: struct.unpack_from("<i", r, 8)[0])
    add(0, 50000, 640); add(0, 50000 + 257 + 639, 2); add(0, 50000 + 257 + 640, 2)   # a gap of just less and just more than window plus slack
    add(0, 99990, 50)                                                            # over the contig's end (no contig ends for the library)
    add(1, 3, 20); add(1, 3, 20, 4); add(1, 4, 20, 0x100); add(1, 5, 20, 0x800)  # a contig change; unmapped and secondary are not covered, supplementary is
    for _ in range(1001):
        add(2, 77, 1)                                                            # depths of 1000 and, a position on, 1001
    for _ in range(1000):
        add(2, 78, 1)
    for _ in range(12):
        add(3, 5, 3)
    for k in range(11):
        add(3, 100 + k, 11 - k)                                                  # depths 1 .. 11
    return tuple(recs)


def check_coverage(lib):
    recs = list(coverage_records())
    whole = check(lib, group(recs), max_len=640)
    assert whole["sorted"] == 1 and whole["cov"][1000] == 1 and whole["cov"][1001] == 1 and whole["cov"][12] >= 3
    coarse = check(lib, group(recs), max_len=640, cov_min=2, cov_max=10, cov_step=3)
    assert coarse["cov"].tolist()[0] > 0 and len(coarse["cov"]) == 5 and coarse["cov"][4] > 0
    for span in (257, 4096):
        got = check(lib, group(recs), max_len=640, span=span)
        assert (got["cov"] == whole["cov"]).all(), span
    blocks, at = [], 0                                                           # the same records in several pushes: chunks of about 20 kB
    while at < len(recs):
        n, size = 0, 0
        while at + n < len(recs) and size < 20000:
            size += len(recs[at + n]); n += 1
        blocks.append(group(recs[at:at + n])); at += n
    assert len(blocks) > 5
    for span in (257, 0):
        got = check(lib, blocks, max_len=640, span=span)
        assert (got["cov"] == whole["cov"]).all(), span


def test_emu_stats_coverage(emu_lib):
    check_coverage(emu_lib)


@pytest.mark.gpu
def test_gpu_stats_coverage(gpu_lib):
    check_coverage(gpu_lib)


# ---- order ----
def check_order(lib):
    recs = [srec(0, 100 + 5 * k, 0x40 if k % 2 else 0x80, [(30, M)], bases(30, k)) for k in range(200)] + [srec(1, 7, 0, [(30, M)], bases(30))]
    want = check(lib, group(recs))
    assert want["sorted"] == 1 and want["cov"].sum() > 0
    inside = recs[:50] + [recs[51], recs[50]] + recs[52:]
    across = [group(recs[:100] + [recs[101]]), group([recs[100]] + recs[102:])]
    tied = recs[:50] + [recs[50]] * 3 + recs[51:]                                    # equal keys are no descent
    assert check(lib, group(tied))["sorted"] == 1
    unmapped_between = recs[:100] + [srec(-1, -1, 4, [], bases(30))] + recs[100:]    # a record that is not covered does not count
    assert check(lib, group(unmapped_between))["sorted"] == 1
    for chunks in ([group(inside)], across):
        got, desc = run(lib, chunks)
        assert got["sorted"] == 0 and sum(desc) == 1 and got["cov"].sum() == 0
        assert [k for k in model.differences(got, want)] == ["sorted", "cov"]
    assert check(lib, [group(recs[150:]), group(recs[:150])])["sorted"] == 0           # a contig that recurs is a descent here


def test_emu_stats_order(emu_lib):
    check_order(emu_lib)


@pytest.mark.gpu
def test_gpu_stats_order(gpu_lib):
    check_order(gpu_lib)


# ---- refusals ----
def check_refusals(lib):
    good = [srec(0, 100 + 3 * k, 0x40, [(5, M), (2, I), (13, M)], bases(20, k), extra=b"NMC\x03") for k in range(70)]
    long_one = bytearray(srec(0, 400, 0, [(20, M)], bases(20))); struct.pack_into("<i", long_one, 20, 4000)
    bad = {   # what, the record, code, words
        "leaves its block_size": (bytes(long_one), SSG_EIO, "malformed record at offset"),
        "mapped without CIGAR": (srec(0, 400, 0, [], bases(20)), SSG_EIO, "is mapped and has no CIGAR"),
        "CIGAR longer than the read": (srec(0, 400, 0x10, [(15, M), (10, I)], bases(20)), SSG_EIO, "puts an insertion or deletion outside the cycles 0 .. 64"),
        "an insertion beyond max_len": (srec(0, 400, 0, [(70, S), (2, I), (3, M)], bases(20)), SSG_EIO, "puts an insertion or deletion outside the cycles 0 .. 64"),
        "unclipped length max_len + 1": (srec(0, 400, 0, [(20, M), (45, H)], bases(20)), SSG_ERANGE, "has an unclipped length above max_len = 64"),
    }
    chunks = [group(good)] + [group(good[:65] + [r] + good[65:]) for r, _, _ in bad.values()] + [group([srec(0, 800, 0, [(20, M), (44, H)], bases(20))])]
    recs, ids = load_chunks(lib, chunks)
    for o in (dict(max_len=0), dict(max_len=65536), dict(n_isize=0), dict(cov_min=-1), dict(cov_min=5, cov_max=4), dict(cov_step=0), dict(span=-1), dict(cov_max=9000)):
        rc, s = capi.stats_create(lib, recs, (), capi.stats_opt(**o))
        assert rc == SSG_EINVAL and s is None and err(lib).startswith("ssg_stats_create: "), o
    for prog, words in ((((1, 0, 0),), "operation 0 underflows the stack"), (((0, 0, 1), (0, 0, 2)), "the filter program leaves 2 values, not exactly one"), (((77, 0, 0),), "operation 0 is the unknown operation 77")):
        rc, s = capi.stats_create(lib, recs, prog)
        assert rc == SSG_EINVAL and err(lib) == "ssg_stats_create: " + words
        assert capi.recs_select(lib, recs, ids[0][0], ids[0][1], prog=prog)[0] == SSG_EINVAL and err(lib) == "ssg_recs_select: " + words
    assert capi.stats_create(lib, None)[0] == SSG_EINVAL
    rc, s = capi.stats_create(lib, recs, (), capi.stats_opt(max_len=64))
    assert rc == 0
    assert capi.stats_push(lib, s, *ids[0]) == (0, 70, 0)
    before = capi.stats_get(lib, s)[1]
    for (what, (_, code, words)), (cid, off) in zip(bad.items(), ids[1:]):
        got = capi.stats_push(lib, s, cid, off)
        assert got[0] == code and err(lib).startswith("ssg_stats_push: ") and words in err(lib), (what, got, err(lib))
        assert model.differences(capi.stats_get(lib, s)[1], before) == [], what
    assert capi.stats_push(lib, s, 99, ids[0][1])[0] == SSG_EINVAL and capi.stats_push(lib, s, ids[0][0], ids[0][1][::-1].copy())[0] == SSG_EINVAL
    assert capi.stats_push(lib, s, *ids[-1]) == (0, 1, 0)                               # an unclipped length of exactly max_len is taken
    assert capi.stats_finish(lib, s) == 0
    assert capi.stats_finish(lib, s) == SSG_EINVAL and "finished already" in err(lib)
    assert capi.stats_push(lib, s, *ids[0])[0] == SSG_EINVAL and "the object is finished" in err(lib)
    after = capi.stats_get(lib, s)[1]
    want = model.compute(ref.records(b"".join(chunks[0] + chunks[-1])), "", max_len=64)
    assert model.differences(after, want) == [] and after["max_len"] == 64
    s.close(); recs.close()


def test_emu_stats_refusals_and_state(emu_lib):
    check_refusals(emu_lib)


@pytest.mark.gpu
def test_gpu_stats_refusals_and_state(gpu_lib):
    check_refusals(gpu_lib)


# ---------------- sambamba stats against samtools 1.3.1 ----------------
SAMTOOLS = os.path.join(ROOT, "oracle", "_ref", "samtools")
CONTIGS = [("sA", 60000), ("sB", 25000)]
READ_LENGTHS = (1, 37, 100, 150, 151, 250, 299, 300, 301, 640)


def write_pairs(path, seed, n_pairs):
    """seeded pairs over two contigs: ten read lengths, reads over a contig's end, CIGARs with S, H, I, D and N, the flags 0x4, 0x8, 0x100, 0x200, 0x400 and 0x800 at
    a few per cent each, `*' sequences and qualities, with and without NM.  Every mapped record has a CIGAR."""
    rng = np.random.RandomState(seed)
    with open(path, "w") as f:
        f.write("@HD\tVN:1.3\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CONTIGS))
        for i in range(n_pairs):
            ctg = int(rng.choice(2, p=[0.7, 0.3]))
            other = 1 - ctg if rng.rand() < 0.04 else ctg
            ln = [int(rng.choice(READ_LENGTHS, p=[0.02, 0.05, 0.3, 0.3, 0.1, 0.1, 0.03, 0.04, 0.03, 0.03])) for _ in range(2)]
            p = [0, 0]
            p[0] = int(rng.randint(1, CONTIGS[ctg][1])) if rng.rand() < 0.97 else CONTIGS[ctg][1] - ln[0] // 2
            p[1] = max(1, min(p[0] + int(rng.randint(-400, 900)), CONTIGS[other][1]))
            rev = [rng.rand() < 0.5, False]
            rev[1] = (not rev[0]) if rng.rand() < 0.85 else rev[0]
            common = 1 | (2 if rng.rand() < 0.8 else 0)
            extra = [sum(b for b in (0x4, 0x8, 0x100, 0x200, 0x400, 0x800) if rng.rand() < 0.03) for _ in range(2)]
            for k in range(2):
                n, flag = ln[k], common | (0x40, 0x80)[k] | (0x10 if rev[k] else 0) | (0x20 if rev[1 - k] else 0) | extra[k]
                if rng.rand() < 0.02:
                    flag &= ~0xc0                                                   # neither first nor last
                kind = int(rng.randint(0, 8)) if n >= 37 else 0
                a = int(rng.randint(5, n - 20)) if n >= 37 else 0
                cigar = ("%dM" % n, "5S%dM" % (n - 5), "%dM2I%dM" % (a, n - a - 2), "%dM3D%dM" % (a, n - a), "%dM120N%dM" % (a, n - a), "%dM1I%dM4D10M2S" % (a, n - a - 13),
                         "%dI%dM" % (2, n - 2), "%dM%dS" % (n - 7, 7))[kind]
                if flag & 0x800 or rng.rand() < 0.02:
                    cigar = "%dH" % int(rng.randint(1, 40)) + cigar + ("%dH" % int(rng.randint(1, 9)) if rng.rand() < 0.5 else "")
                if flag & 4 and rng.rand() < 0.5:
                    cigar = "*"
                star = rng.rand() < 0.02
                seq = "*" if star else "".join("ACGTNRY="[b] for b in rng.choice(8, size=n, p=[0.24, 0.25, 0.25, 0.22, 0.02, 0.005, 0.005, 0.01]))
                qual = "*" if star or rng.rand() < 0.03 else "".join(chr(33 + v) for v in rng.choice([41, 40, 37, 30, 20, 12, 2, 0, 60, 93], size=n))
                isize = 0 if ctg != other else (p[1 - k] - p[k] + (ln[1 - k] if p[1 - k] >= p[k] else -ln[k])) * (1 if rng.rand() < 0.98 else 17)
                tags = "\tNM:i:%d" % rng.randint(0, 9) if rng.rand() < 0.7 else ""
                tags += "\tXS:Z:abc\tXB:B:c,1,2,3" if rng.rand() < 0.2 else ""
                f.write("p%d\t%d\t%s\t%d\t%d\t%s\t%s\t%d\t%d\t%s\t%s%s\n" % (i, flag, CONTIGS[ctg if k == 0 else other][0], p[k], int(rng.choice([0, 7, 30, 60])), cigar,
                                                                      "=" if ctg == other else CONTIGS[other if k == 0 else ctg][0], p[1 - k], isize, seq, qual, tags))


class StatsFile:
    """a BAM of about 3000 pairs as `samtools sort' wrote it and in generation order, both in blocks that begin at records, and every run of `stats' on them"""

    def __init__(self, sambamba, d):
        self.sambamba, self.d, self.runs = sambamba, str(d), {}
        self.clean = {k: v for k, v in os.environ.items() if k not in OURS + KNOBS + ("SSG_STATS_SPAN", "SSG_PROF")}
        assert os.path.exists(SAMTOOLS)
        write_pairs(self.d + "/in.sam", 31, 3000)
        self.samtools("view", "-b", "-o", "in.u.bam", "in.sam")
        self.samtools("sort", "-o", "st.bam", "in.u.bam")
        open(self.d + "/sorted.bam", "wb").write(reblock(open(self.d + "/st.bam", "rb").read()))
        open(self.d + "/unsorted.bam", "wb").write(reblock(open(self.d + "/in.u.bam", "rb").read()))
        open(self.d + "/skew.bam", "wb").write(reblock(open(self.d + "/st.bam", "rb").read(), step=3001))

    def run(self, args, extra=None):
        key = (tuple(args), tuple(sorted((extra or {}).items())))
        if key not in self.runs:
            env = dict(self.clean)
            env.update(extra or {})
            r = subprocess.run([self.sambamba, "stats"] + [self.d + "/" + a if a.endswith(".bam") and "/" not in a else a for a in args], capture_output=True, env=env)
            r.stderr = r.stderr.decode()
            self.runs[key] = r
        return self.runs[key]

    def out(self, args, extra=None):
        r = self.run(args, extra)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.decode()

    def samtools(self, *args):
        r = subprocess.run([SAMTOOLS] + list(args), capture_output=True, cwd=self.d)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.decode()


@pytest.fixture(scope="module")
def emu_stats(tmp_path_factory, emu_lib):
    return StatsFile(os.path.join(ROOT, "tests", "emu", "sambamba_emu"), tmp_path_factory.mktemp("stats_emu"))


@pytest.fixture(scope="module")
def gpu_stats(tmp_path_factory, gpu_lib):
    return StatsFile(os.path.join(ROOT, "bin", "sambamba"), tmp_path_factory.mktemp("stats_gpu"))


def numbers(text, drop=("GCD",)):
    """the lines that are neither comments nor of a dropped section, without their trailing comments"""
    return [l.split("\t# ")[0] for l in text.splitlines() if not l.startswith("#") and l.split("\t")[0] not in drop]


RUNS = {   # name -> (ours, samtools')
    "plain": ([], []),
    "no_duplicates": (["-F", "not duplicate"], ["-d"]),
    "paired": (["-F", "paired"], ["-f", "1"]),
    "coverage_bins": (["-c", "2,10,3"], ["-c", "2,10,3"]),
    "insert_sizes": (["-i", "500"], ["-i", "500"]),
    "main_bulk": (["-m", "0.5"], ["-m", "0.5"]),
    "sparse": (["-x"], ["-x"]),
}


def check_command(v, name):
    ours, theirs = RUNS[name]
    got, want = numbers(v.out(ours + ["sorted.bam"])), numbers(v.samtools("stats", *(theirs + ["sorted.bam"])))
    assert len(want) > 1500 and [l for l in want if l.startswith("SN\tis sorted:")] == ["SN\tis sorted:\t1"]
    assert [l.split("\t")[0] for l in want].count("SN") == 31 and {"CHK", "FFQ", "LFQ", "GCF", "GCL", "GCC", "IS", "RL", "ID", "IC", "COV"} <= {l.split("\t")[0] for l in want}
    assert got == want, [(a, b) for a, b in zip(got, want) if a != b][:5]
    if name == "plain":                                                      # the same records in generation order: everything but COV
        text = v.out(["unsorted.bam"])
        got, want = numbers(text, ("GCD", "COV")), numbers(v.samtools("stats", "unsorted.bam"), ("GCD", "COV"))
        assert "SN\tis sorted:\t0" in got and got == want and "# COV is not computed" in text and not [l for l in text.splitlines() if l.startswith("COV")]
        for knobs in ({"SSG_STATS_SPAN": "257"}, {"SSG_STATS_TILE": "5", "SSG_STATS_SLAB": "77"}):
            assert v.out(["sorted.bam"], knobs) == v.out(["sorted.bam"])
        text = v.out(["sorted.bam"])
        assert text.count("\n# ") + 1 == len([l for l in text.splitlines() if l.startswith("#")]) and "# GCD is not computed" in text


@pytest.mark.parametrize("name", sorted(RUNS))
def test_emu_stats_command_agrees_with_samtools(emu_stats, name):
    check_command(emu_stats, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RUNS))
def test_gpu_stats_command_agrees_with_samtools(gpu_stats, name):
    check_command(gpu_stats, name)


def check_command_refusals(v):
    for args, words in ((["skew.bam"], "skew.bam is "), (["--max-read-length", "300", "sorted.bam"], "has an unclipped length above max_len = 300"), (["-F", "read_name == 3", "sorted.bam"], "is not supported by this filter"),
                        (["-c", "5,4,1", "sorted.bam"], "-c takes"), (["-r", "ref.fa", "sorted.bam"], "unsupported option -r"), (["sorted.bam", "sA:1-100"], "regions are not supported")):
        r = v.run(args)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.count("\n") == 1 and r.stderr.startswith("[sambamba] ") and words in r.stderr, (args, r.stderr)
    with open(v.d + "/sorted.bam", "rb") as f:
        r = subprocess.run([v.sambamba, "stats", "/dev/stdin"], input=f.read(), capture_output=True, env=v.clean)
    assert r.returncode == 1 and b"not a regular file" in r.stderr and r.stderr.count(b"\n") == 1
    r = v.run(["sorted.bam"], {"SSG_PROF": "1"})
    assert r.returncode == 0 and all("kernel ssg_k_stats_%s" % k in r.stderr for k in ("decide", "bases", "crc", "cov_add", "cov_hist")) if "emu" not in v.sambamba else r.returncode == 0


def test_emu_stats_command_refusals(emu_stats):
    check_command_refusals(emu_stats)


@pytest.mark.gpu
def test_gpu_stats_command_refusals(gpu_stats):
    check_command_refusals(gpu_stats)
