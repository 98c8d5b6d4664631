"""The sorted records gathered on the device (k_rec_gather.h; ssg_recs_*, ssg_bgzf_compress_recs): the gather kernel against a slice
of the concatenated records at every alignment of destination and source, the edges of the record store, ssg_bgzf_compress_recs against ssg_bgzf_compress
on the host-gathered payload, and `sambamba sort` writing the same file and index with SSG_SORT_DEVICE_GATHER=1, with every one of its fall-backs, and the
same log without it.  CPU-side on the host emulation of the kernels; `-m gpu` on the MI355X."""
import ctypes as C
import functools
import gzip
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from common import ROOT
from speedseq_amd import capi

SSG_ENOMEM, SSG_EINVAL, SSG_EOVERFLOW = -12, -22, -75
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
LENGTHS = [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 0xff01, 200003]
MAX_PAYLOAD = 0xff00


def bam_record(rng, l_seq=150):
    name = b"read%d\0" % rng.randint(10 ** 7)
    core = struct.pack("<iiIIiiii", rng.randint(25), rng.randint(10 ** 8), (len(name) | 60 << 8 | 4681 << 16), (99 << 16) | 1, l_seq, rng.randint(25), rng.randint(10 ** 8), rng.randint(-500, 500))
    body = (core + name + struct.pack("<I", l_seq << 4) + rng.bytes((l_seq + 1) // 2) + rng.choice(np.array([40, 40, 40, 37, 12], dtype=np.uint8), l_seq).tobytes()
            + b"NMC\x00MDZ150\x00ASC\x96XSC\x00RGZgrp1\x00MCZ150M\x00MQC\x3c")
    return struct.pack("<I", len(body)) + body


@functools.lru_cache(maxsize=None)
def bam_stream():
    """BAM-shaped records, a little over the longest record of the tests"""
    rng = np.random.RandomState(11)
    recs, total = [], 0
    while total < 200003 + 37 * 64:
        recs.append(bam_record(rng))
        total += len(recs[-1])
    return b"".join(recs)


class Stream:
    """records as five chunks of uneven size, and the stream a seeded permutation makes of them"""

    def __init__(self, records, seed, n_chunks=5):
        rng = np.random.RandomState(seed)
        bounds = sorted(set([0, len(records)] + [int(x) for x in rng.choice(np.arange(1, len(records)), size=min(n_chunks - 1, len(records) - 1), replace=False)]))
        self.chunks, loc = [], []
        for c, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
            o = 0
            for r in records[a:b]:
                loc.append(c << 40 | o)
                o += len(r)
            self.chunks.append(b"".join(records[a:b]))
        perm = rng.permutation(len(records))
        self.sorted = [records[i] for i in perm]
        self.loc = np.array([loc[i] for i in perm], dtype=np.uint64)
        self.cum = np.zeros(len(records) + 1, dtype=np.uint64)
        self.cum[1:] = np.cumsum([len(r) for r in self.sorted])
        self.whole = b"".join(self.sorted)
        # address of a record's first byte modulo 16 (a chunk's device allocation is at least 256-byte aligned)
        self.src16 = np.array([int(l) & 15 for l in self.loc])

    def upload(self, lib, cap=None, order=True):
        recs = capi.recs_create(lib, sum(len(c) for c in self.chunks) if cap is None else cap)
        for k, c in enumerate(self.chunks):
            assert capi.recs_append(lib, recs, c) == k
        if order:
            capi.recs_order(lib, recs, self.loc, self.cum)
        return recs


@functools.lru_cache(maxsize=None)
def length_stream():
    rng = np.random.RandomState(23)
    records = []
    for k, n in enumerate(LENGTHS):
        records += [rng.bytes(n), bam_stream()[37 * k:37 * k + n]]
    assert all(len(r) >= 1 for r in records) and len(records) == 2 * len(LENGTHS)
    return Stream(records, seed=29)


def gather(lib, recs, v0, v1):
    """recs_gather into a buffer filled with 0xAB: the bytes, after checking that nothing behind v1 - v0 was touched"""
    out = np.full(v1 - v0 + 64, 0xAB, dtype=np.uint8)
    got = capi.recs_gather(lib, recs, v0, v1, out=out)
    assert (out[v1 - v0:] == 0xAB).all(), (v0, v1, out[v1 - v0:].tobytes().hex())
    return got.tobytes()


def check_gather(lib):
    st = length_stream()
    recs = st.upload(lib)
    total = len(st.whole)
    assert int(st.cum[-1]) == total
    assert gather(lib, recs, 0, total) == st.whole                                    # the whole stream
    for v in (0, 1, 4097, total):
        assert gather(lib, recs, v, v) == b""                                         # v0 == v1 writes nothing
    rng = np.random.RandomState(31)
    ranges, seen = [], set()
    # ranges that begin and end inside a record: in the long ones, across several, and within a single granule
    big = [i for i in range(len(st.sorted)) if len(st.sorted[i]) >= 4095]
    for i in big:
        a, b = int(st.cum[i]), int(st.cum[i + 1])
        ranges += [(a + 1, b - 1), (a + int(rng.randint(1, 4000)), a + 4090), (a + 5, a + 14)]
    for _ in range(12):
        a, b = sorted(int(x) for x in rng.randint(0, total + 1, size=2))
        ranges.append((a, b))
    # every combination class of (v0 % 16, first source address % 16): v0 = a record's start + k, the first source byte is that record's byte k
    for i in range(len(st.sorted)):
        for k in range(min(len(st.sorted[i]), 16)):
            v0 = int(st.cum[i]) + k
            key = (v0 % 16, (int(st.src16[i]) + k) % 16)
            if key not in seen and (sum(1 for s in seen if s[0] == key[0]) < 2 or sum(1 for s in seen if s[1] == key[1]) < 2):
                seen.add(key)
                ranges.append((v0, min(total, v0 + int(rng.randint(1, 9000)))))
    assert set(k[0] for k in seen) == set(range(16)), sorted(seen)                   # v0 falls on every alignment ...
    assert set(k[1] for k in seen) == set(range(16)), sorted(seen)                   # ... and so does the first source address
    for v0, v1 in ranges:
        assert gather(lib, recs, v0, v1) == st.whole[v0:v1], (v0, v1)
    recs.close()


def test_emu_gather_matches_a_slice_of_the_concatenation(emu_lib):
    check_gather(emu_lib)


@pytest.mark.gpu
def test_gpu_gather_matches_a_slice_of_the_concatenation(gpu_lib):
    check_gather(gpu_lib)


def check_store_edges(lib):
    st = length_stream()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    # an append past cap_bytes: SSG_ENOMEM, and the earlier chunks still gather
    four = sum(len(c) for c in st.chunks[:4])
    recs = capi.recs_create(lib, four + len(st.chunks[4]) - 1)
    for k in range(4):
        assert capi.recs_append(lib, recs, st.chunks[k]) == k
    last = np.frombuffer(st.chunks[4], dtype=np.uint8)
    assert lib.l.ssg_recs_append(recs.h, ptr(last), C.c_uint64(last.size), None) == SSG_ENOMEM
    assert b"capacity" in lib.l.ssg_last_error()
    keep = [i for i in range(len(st.loc)) if int(st.loc[i]) >> 40 < 4]
    loc = st.loc[keep]
    cum = np.zeros(len(keep) + 1, dtype=np.uint64)
    cum[1:] = np.cumsum([len(st.sorted[i]) for i in keep])
    capi.recs_order(lib, recs, loc, cum)
    want = b"".join(st.sorted[i] for i in keep)
    assert gather(lib, recs, 0, len(want)) == want
    assert gather(lib, recs, 3, len(want) - 5) == want[3:-5]

    # what ssg_recs_order refuses, each with a message
    def refused(loc, cum, word):
        loc, cum = np.ascontiguousarray(loc, dtype=np.uint64), np.ascontiguousarray(cum, dtype=np.uint64)
        assert lib.l.ssg_recs_order(recs.h, ptr(loc), ptr(cum), C.c_int64(len(loc))) == SSG_EINVAL
        assert word in lib.l.ssg_last_error(), lib.l.ssg_last_error()
    c1 = cum.copy(); c1[0] = 1
    refused(loc, c1, b"cum[0]")
    c2 = cum.copy(); c2[5] = c2[4] - 1
    refused(loc, c2, b"decreases")
    l3 = loc.copy(); l3[7] = np.uint64(4 << 40)                                     # (the fifth chunk was refused)
    refused(l3, cum, b"chunk 4")
    c = max(range(4), key=lambda k: len(st.chunks[k]))
    clen = len(st.chunks[c])
    assert clen > 9
    refused([c << 40 | (clen - 9)], [0, 10], b"past the end")                         # one byte past its chunk
    capi.recs_order(lib, recs, [c << 40 | (clen - 9)], [0, 9])                        # ... and up to its last byte
    assert gather(lib, recs, 0, 9) == st.chunks[c][-9:]
    capi.recs_order(lib, recs, loc, cum)                                              # a refused order leaves the store usable
    assert gather(lib, recs, 0, len(want)) == want
    # a range beyond the stream
    out = np.full(len(want) + 64, 0xAB, dtype=np.uint8)
    assert lib.l.ssg_recs_gather(recs.h, C.c_uint64(0), C.c_uint64(len(want) + 1), ptr(out)) == SSG_EINVAL
    assert lib.l.ssg_recs_gather(recs.h, C.c_uint64(5), C.c_uint64(4), ptr(out)) == SSG_EINVAL
    assert (out == 0xAB).all()
    # no record at all
    capi.recs_order(lib, recs, [], [0])
    assert gather(lib, recs, 0, 0) == b""
    assert lib.l.ssg_recs_gather(recs.h, C.c_uint64(0), C.c_uint64(1), ptr(out)) == SSG_EINVAL
    recs.close()
    empty = capi.recs_create(lib, 0)
    capi.recs_order(lib, empty, [], [0])
    empty.close()


def test_emu_record_store_edges(emu_lib):
    check_store_edges(emu_lib)


@pytest.mark.gpu
def test_gpu_record_store_edges(gpu_lib):
    check_store_edges(gpu_lib)


def cut_like_write_sorted(cum):
    """the block cuts of write_sorted (sambamba_main.cpp): a record does not straddle blocks unless it is larger than one"""
    cut, open_ = [0], 0
    for i in range(len(cum) - 1):
        c0, c1 = int(cum[i]), int(cum[i + 1])
        if c0 > open_ and c0 - open_ + (c1 - c0) > MAX_PAYLOAD:
            cut.append(c0); open_ = c0
        while c1 - open_ >= MAX_PAYLOAD:
            open_ += MAX_PAYLOAD; cut.append(open_)
    if int(cum[-1]) > cut[-1]:
        cut.append(int(cum[-1]))
    return np.array(cut, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def block_sets():
    rng = np.random.RandomState(37)
    sets = {}
    # BAM-shaped records of about 350 bytes, cut as write_sorted cuts them: 40 blocks
    records, total = [], 0
    while True:
        r = bam_record(rng, l_seq=int(rng.randint(120, 180)))
        if total + len(r) > 40 * MAX_PAYLOAD - 20000:
            break
        records.append(r); total += len(r)
    st = Stream(records, seed=41)
    sets["bam"] = (st, cut_like_write_sorted(st.cum))
    # one record of 200003 bytes that spans four blocks, between small ones
    small = [bam_record(rng) for _ in range(40)]
    st = Stream(small[:20] + [bam_stream()[:200003]] + small[20:], seed=43)
    st.sorted_fix = None
    sets["long"] = (st, cut_like_write_sorted(st.cum))
    # 4096 blocks of three bytes and one of the largest size behind them: the second device call's
    st = Stream([rng.bytes(3) for _ in range(4096)] + [bam_stream()[5 * 37:5 * 37 + 0xff00]], seed=47)
    order = np.argsort([len(r) for r in st.sorted], kind="stable")                    # (the large one last in the stream)
    st.sorted = [st.sorted[i] for i in order]; st.loc = st.loc[order]
    st.cum[1:] = np.cumsum([len(r) for r in st.sorted]); st.whole = b"".join(st.sorted)
    sets["batch"] = (st, st.cum.copy())
    return sets


def check_compress_recs(lib, name):
    st, cut = block_sets()[name]
    n = len(cut) - 1
    steps = np.diff(cut.astype(np.int64))
    if name == "bam":
        assert n == 40
    if name == "long":
        assert int((steps == MAX_PAYLOAD).sum()) == 3 and 200003 > 3 * MAX_PAYLOAD     # the long record lies in four blocks
    if name == "batch":
        assert n == 4097 and int(steps[-1]) == 0xff00
    recs = st.upload(lib)
    want, want_off, want_crc = capi.bgzf_compress(lib, st.whole, cut)
    got, off, crc = capi.bgzf_compress_recs(lib, recs, cut)
    assert (off == want_off).all() and (crc == want_crc).all()
    assert got.tobytes() == want.tobytes()
    whole = got.tobytes()
    for b in range(n):                                                                # every member inflates to its payload
        assert gzip.decompress(whole[int(off[b]):int(off[b + 1])]) == st.whole[int(cut[b]):int(cut[b + 1])], b
    if name == "bam":
        # a stretch of the blocks: absolute offsets that do not start at 0
        got2, off2, crc2 = capi.bgzf_compress_recs(lib, recs, cut[7:19])
        assert got2.tobytes() == whole[int(off[7]):int(off[18])] and (crc2 == crc[7:18]).all()
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        # no block: out_off[0] = 0 and nothing else
        o1 = np.full(1, 77, dtype=np.uint64); out = np.full(64, 0xAB, dtype=np.uint8)
        assert lib.l.ssg_bgzf_compress_recs(recs.h, ptr(cut), C.c_long(0), ptr(out), C.c_uint64(0), ptr(o1), None) == 0
        assert int(o1[0]) == 0 and (out == 0xAB).all()
        # a step above 0xff00
        bad = np.array([0, 0xff01], dtype=np.uint64); o2 = np.zeros(2, dtype=np.uint64); out = np.zeros(0xff01 + 64, dtype=np.uint8)
        assert lib.l.ssg_bgzf_compress_recs(recs.h, ptr(bad), C.c_long(1), ptr(out), C.c_uint64(out.size), ptr(o2), None) == SSG_EINVAL
        assert b"0xff00" in lib.l.ssg_last_error()
        # out_cap one byte short: SSG_EOVERFLOW and nothing behind it; the exact size is enough
        cap = len(whole) - 1
        out = np.full(cap + 64, 0xAB, dtype=np.uint8); o3 = np.zeros(n + 1, dtype=np.uint64)
        assert lib.l.ssg_bgzf_compress_recs(recs.h, ptr(cut), C.c_long(n), ptr(out), C.c_uint64(cap), ptr(o3), None) == SSG_EOVERFLOW
        assert (out[cap:] == 0xAB).all()
        out = np.full(cap + 1 + 64, 0xAB, dtype=np.uint8)
        assert lib.l.ssg_bgzf_compress_recs(recs.h, ptr(cut), C.c_long(n), ptr(out), C.c_uint64(cap + 1), ptr(o3), None) == 0
        assert out[:cap + 1].tobytes() == whole and (out[cap + 1:] == 0xAB).all()
    recs.close()


@pytest.mark.parametrize("name", ["bam", "long", "batch"])
def test_emu_bgzf_compress_recs_equals_bgzf_compress(emu_lib, name):
    check_compress_recs(emu_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bam", "long", "batch"])
def test_gpu_bgzf_compress_recs_equals_bgzf_compress(gpu_lib, name):
    check_compress_recs(gpu_lib, name)


def write_sam(path):
    """the 6000 records of test_bgzf_frame.py's generator (three contigs, mates pointing at one another, unmapped reads among them and at the end) and one
    with 70 000 bases: a record that is split over blocks"""
    rng = np.random.RandomState(17)
    ctg = [("ctgA", 400000), ("ctgB", 250000), ("ctgC", 90000)]
    with open(path, "w") as f:
        f.write("@HD\tVN:1.3\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in ctg) + "@RG\tID:g\tSM:s\n")
        for i in range(3000):
            seq = ["".join("ACGT"[b] for b in rng.randint(0, 4, size=100)) for _ in range(2)]
            qual = ["".join(chr(33 + q) for q in rng.choice([40, 40, 37, 12], size=100)) for _ in range(2)]
            if i % 11 == 0:                                       # neither end mapped
                for e in range(2):
                    f.write("p%d\t%d\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\tRG:Z:g\n" % (i, 77 if e == 0 else 141, seq[e], qual[e]))
                continue
            name, ln = ctg[rng.randint(3)]
            p1 = int(rng.randint(1, ln - 700)); p2 = p1 + int(rng.randint(50, 500))
            if i % 7 == 0:                                        # the mate unmapped, placed with its mate
                f.write("p%d\t73\t%s\t%d\t60\t100M\t=\t%d\t0\t%s\t%s\tNM:i:0\tRG:Z:g\n" % (i, name, p1, p1, seq[0], qual[0]))
                f.write("p%d\t133\t%s\t%d\t0\t*\t=\t%d\t0\t%s\t%s\tRG:Z:g\n" % (i, name, p1, p1, seq[1], qual[1]))
                continue
            f.write("p%d\t99\t%s\t%d\t60\t100M\t=\t%d\t%d\t%s\t%s\tNM:i:1\tRG:Z:g\n" % (i, name, p1, p2, p2 + 100 - p1, seq[0], qual[0]))
            f.write("p%d\t147\t%s\t%d\t60\t60M2D40M\t=\t%d\t%d\t%s\t%s\tNM:i:2\tRG:Z:g\n" % (i, name, p2, p1, p1 - p2 - 100, seq[1], qual[1]))
            if i == 1500:
                big = "".join("ACGT"[b] for b in rng.randint(0, 4, size=70000))
                f.write("long\t0\tctgB\t120000\t60\t70000M\t*\t0\t0\t%s\t%s\tRG:Z:g\n" % (big, "".join(chr(33 + q) for q in rng.choice([40, 37, 12], size=70000))))


BASE_ENV = {"SSG_BGZF_DEVICE": "1", "SSG_SORT_DEV_BATCH": "16", "SSG_SORT_IN_CHUNK_BYTES": "300000", "SSG_SORT_LOG": "1"}
OURS = ("SSG_SORT_DEVICE_GATHER", "SSG_SORT_DEVICE_POOL_MB", "SSG_BGZF_DEVICE_CRC", "SSG_SORT_CHUNK_BYTES", "SSG_BGZF_FAIL_AFTER", "SSG_SORT_HOST_BATCHES", "SSG_SORT_PRODUCERS",
        "SSG_SORT_DEVICES", "SSG_BAM_LEVEL", "SSG_SORT_NO_BAI", "SSG_DEBUG")


class Sorter:
    """one unsorted BAM per session and binary; every run of `sambamba sort` on it under another environment"""

    def __init__(self, sambamba, d):
        self.sambamba, self.d, self.runs = sambamba, str(d), {}
        write_sam(self.d + "/in.sam")
        with open(self.d + "/in.sam", "rb") as fi, open(self.d + "/u.bam", "wb") as fo:
            subprocess.run([sambamba, "view", "-S", "-f", "bam", "-l", "0", "/dev/stdin"], stdin=fi, stdout=fo, check=True)

    def run(self, tag, extra):
        if tag not in self.runs:
            env = {k: v for k, v in os.environ.items() if k not in OURS}
            env.update(BASE_ENV); env.update(extra)
            out = "%s/%s.bam" % (self.d, tag)
            r = subprocess.run([self.sambamba, "sort", "-t", "4", "-m", "1G", "--tmpdir=%s/tmp_%s" % (self.d, tag), "-o", out, self.d + "/u.bam"], check=True, capture_output=True, text=True, env=env)
            self.runs[tag] = (open(out, "rb").read(), open(out + ".bai", "rb").read(), r.stderr)
        return self.runs[tag]


@pytest.fixture(scope="module")
def emu_sorter(tmp_path_factory, emu_lib):
    return Sorter(os.path.join(ROOT, "tests", "emu", "sambamba_emu"), tmp_path_factory.mktemp("sort_device_gather_emu"))


@pytest.fixture(scope="module")
def gpu_sorter(tmp_path_factory, gpu_lib):
    return Sorter(os.path.join(ROOT, "bin", "sambamba"), tmp_path_factory.mktemp("sort_device_gather_gpu"))


def deflated_line(log):
    line = [l for l in log.split("\n") if "blocks deflated on" in l]
    assert len(line) == 1, log[-1500:]
    return line[0]


def check_sort_same_file(sorter):
    dev_bam, dev_bai, dev_log = sorter.run("gather_dev", {"SSG_SORT_DEVICE_GATHER": "1"})
    host_bam, host_bai, host_log = sorter.run("gather_host", {})
    assert dev_bam == host_bam and dev_bai == host_bai                              # the same file, byte for byte, and the same index
    assert "gather on the device" in deflated_line(dev_log) and "gather on the host" not in deflated_line(dev_log), dev_log[-1500:]
    assert "gather on the host" in deflated_line(host_log) and "gather on the device" not in host_log, host_log[-1500:]
    assert "device gather off" not in dev_log and "device gather" not in host_log
    assert int(re.search(r"write of (\d+) blocks", dev_log).group(1)) > 16, dev_log[-1500:]       # more than one batch
    assert int(re.search(r"device gather: (\d+) chunks", dev_log).group(1)) > 1, dev_log[-1500:]   # more than one chunk
    assert dev_bam.endswith(EOF_MARKER)
    plain = gzip.decompress(dev_bam)                                                  # every member's CRC-32 and ISIZE hold
    assert plain[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", plain, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", plain, o); o += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", plain, o); o += 8 + l_name
    keys, sizes = [], []
    while o < len(plain):
        bs, tid, pos = struct.unpack_from("<iii", plain, o)
        keys.append((tid if tid >= 0 else 1 << 30, pos)); sizes.append(bs); o += 4 + bs
    assert len(keys) == 6001 and keys == sorted(keys) and keys[-1][0] == 1 << 30 and keys[0][0] == 0
    assert max(sizes) > MAX_PAYLOAD                                                   # a record split over blocks


def test_emu_sambamba_sort_same_file_with_device_gather(emu_sorter):
    check_sort_same_file(emu_sorter)


@pytest.mark.gpu
def test_gpu_sambamba_sort_same_file_with_device_gather(gpu_sorter):
    check_sort_same_file(gpu_sorter)


FALLBACKS = {
    "pool": ({"SSG_SORT_DEVICE_POOL_MB": "1"}, r"device gather off \(.*capacity", "gather on the host"),
    "crc": ({"SSG_BGZF_DEVICE_CRC": "0"}, r"device gather off \(SSG_BGZF_DEVICE_CRC=0", "gather + CRC-32 on the host"),
    "spill": ({"SSG_SORT_CHUNK_BYTES": "700000"}, r"device gather off \(.*spilled", None),
    "fail": ({"SSG_BGZF_FAIL_AFTER": "1"}, r"BGZF deflate on the device failed: \(SSG_BGZF_FAIL_AFTER: test\)", "gather on the device"),
}


def check_fallback(sorter, name):
    extra, reason, where = FALLBACKS[name]
    host_bam, host_bai, _ = sorter.run("gather_host", {})
    bam, bai, log = sorter.run("fallback_" + name, dict(extra, SSG_SORT_DEVICE_GATHER="1"))
    assert len([l for l in log.split("\n") if re.search(reason, l)]) == 1, log[-1500:]   # one line names the reason
    if name == "spill":
        assert "sorted runs merged" in log and "gather on the device" not in log, log[-1500:]
        assert bam == host_bam and bai == host_bai
    else:
        assert where in deflated_line(log), log[-1500:]
        if name == "fail":
            # the host's pool (zlib) finishes the file -- other deflate streams than the device's, and which batch the device still made is a race of the producers,
            # with the switch as without it: the members differ from the host run's, the records in them do not
            assert "compressing the rest of the output on the host" in log
            assert bam.endswith(EOF_MARKER) and gzip.decompress(bam) == gzip.decompress(host_bam)
        else:
            assert bam == host_bam and bai == host_bai


@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_emu_sambamba_sort_fallbacks_write_the_same_file(emu_sorter, name):
    check_fallback(emu_sorter, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_gpu_sambamba_sort_fallbacks_write_the_same_file(gpu_sorter, name):
    check_fallback(gpu_sorter, name)


# the SSG_SORT_LOG lines of this sort before the switch existed, numbers replaced by `#'
LOG_BEFORE = """[sambamba] sort: write: offsets and block cuts # s, gather + deflate + write of # blocks # s (record view for the index # s, # workers started in # s; writer: waited # s for blocks, wrote for # s; per worker: gather # s, deflate # s, held back by the writer's window # s)
[sambamba] sort: write: blocks deflated on # device(s) (# producer threads; `gather' = gather on the host, `deflate' = upload + kernels + download: CRC-# on the device, framing too)
[sambamba] sort: write: index finished # s after the last block (its thread waited # s for block offsets)
[sambamba] sort: # records, # GB: input # s (from start), device sort of the keys # s, gather + deflate (level #, # threads) + write # s"""


def normalise(log):
    return [re.sub(r"\d+(\.\d+)?", "#", l) for l in log.split("\n") if l.startswith("[sambamba]")]


def check_log_unset(sorter):
    _, _, log = sorter.run("gather_host", {})
    lines = normalise(log)
    assert sum(1 for l in lines if l.endswith("; gather on the host")) == 1
    assert [l[:-len("; gather on the host")] if l.endswith("; gather on the host") else l for l in lines] == LOG_BEFORE.split("\n"), "\n".join(lines)


def test_emu_sambamba_sort_log_without_the_switch(emu_sorter):
    check_log_unset(emu_sorter)


@pytest.mark.gpu
def test_gpu_sambamba_sort_log_without_the_switch(gpu_sorter):
    check_log_unset(gpu_sorter)
