"""Complete BGZF members from the device (k_bgzf_frame.h; ssg_crc32_batch, ssg_bgzf_compress, ssg_bgzf_bound): the CRC-32
kernel against zlib.crc32 at every boundary of its lane split, the framed members against Python's gzip (which verifies CRC-32 and ISIZE), the
end-of-file marker, the edges of the entry point, the per-call batch, and `sambamba sort` writing the same file with the device's checksums
as with the host's.  CPU-side on the host emulation of the kernels; `-m gpu` on the MI355X."""
import ctypes as C
import functools
import gzip
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from common import ROOT
from speedseq_amd import capi

EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
HDR16 = bytes.fromhex("1f8b08040000000000ff060042430200")
LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 0xfeff, 0xff00, 65537, 200003, (1 << 20) + 3]
BLOCK_LENGTHS = [n for n in LENGTHS if n <= 0xff00]
SSG_EINVAL, SSG_EOVERFLOW = -22, -75


@functools.lru_cache(maxsize=None)
def bam_stream():
    """BAM-shaped records (core, name, CIGAR, packed bases, qualities of few values, tags), a little over the longest range"""
    rng = np.random.RandomState(11)
    recs, total = [], 0
    while total < (1 << 20) + 4096:
        name = b"read%d\0" % rng.randint(10 ** 7)
        core = struct.pack("<iiIIiiii", rng.randint(25), rng.randint(10 ** 8), 0x12345678, (99 << 16) | 1, 150, rng.randint(25), rng.randint(10 ** 8), rng.randint(-500, 500))
        body = core + name + struct.pack("<I", 150 << 4) + rng.bytes(75) + rng.choice(np.array([40, 40, 40, 37, 12], dtype=np.uint8), 150).tobytes() + b"NMC\x00MDZ150\x00ASC\x96XSC\x00RGZgrp1\x00MCZ150M\x00MQC\x3c"
        recs.append(struct.pack("<I", len(body)) + body)
        total += len(recs[-1])
    return b"".join(recs)


def bam_shaped(n, k):
    return bam_stream()[37 * k:37 * k + n]          # (a window that starts inside a record, a different one per case)


def text_shaped(rng, n):
    parts, total = [], 0
    while total < n:
        parts.append([b"@r%d/1\n" % rng.randint(999), b"ACGTTGCA" * rng.randint(1, 13) + b"\n", b"+\n", b"IIIIHHHGG#" * rng.randint(1, 10) + b"\n"][rng.randint(4)])
        total += len(parts[-1])
    return b"".join(parts)[:n]


def run_shaped(rng, n):
    vals = rng.randint(0, 256, size=n // 2 + 1).astype(np.uint8)
    return np.repeat(vals, rng.randint(1, 300, size=len(vals)))[:n].tobytes()


@functools.lru_cache(maxsize=None)
def crc_cases():
    """the ranges of the CRC-32 test and zlib's answer for each: every length as zeros, 0xff, noise and BAM-shaped records (zeros and 0xff: the
    checksum then depends on the length alone, so a wrong shift in the combine shows), one empty range more between two that are not"""
    rng = np.random.RandomState(5)
    ranges = []
    for k, n in enumerate(LENGTHS):
        ranges += [bytes(n), b"\xff" * n, rng.bytes(n), bam_shaped(n, k)]
    ranges.insert(len(ranges) - 1, b"")
    assert ranges[-3] and not ranges[-2] and ranges[-1]
    return ranges, [zlib.crc32(r) for r in ranges]


def concat(ranges):
    cut = np.zeros(len(ranges) + 1, dtype=np.uint64)
    cut[1:] = np.cumsum([len(r) for r in ranges])
    return np.frombuffer(b"".join(ranges), dtype=np.uint8), cut


def check_crc32_batch(lib):
    ranges, want = crc_cases()
    data, cut = concat(ranges)
    starts = set(int(c) % 8 for c, r in zip(cut[:-1], ranges) if r)
    assert starts == set(range(8)), starts                       # the cuts fall on every alignment
    got = capi.crc32_batch(lib, data, cut)
    bad = [(i, len(ranges[i]), hex(int(got[i])), hex(want[i])) for i in range(len(ranges)) if int(got[i]) != want[i]]
    assert not bad, bad[:8]
    # the same ranges in reverse order of size: other starts, other neighbours, the same answers
    order = sorted(range(len(ranges)), key=lambda i: -len(ranges[i]))
    data2, cut2 = concat([ranges[i] for i in order])
    got2 = capi.crc32_batch(lib, data2, cut2)
    bad = [(i, len(ranges[i]), hex(int(g)), hex(want[i])) for i, g in zip(order, got2) if int(g) != want[i]]
    assert not bad, bad[:8]
    assert len(capi.crc32_batch(lib, b"", [0])) == 0            # no range at all


def test_emu_crc32_batch_matches_zlib(emu_lib):
    check_crc32_batch(emu_lib)


@pytest.mark.gpu
def test_gpu_crc32_batch_matches_zlib(gpu_lib):
    check_crc32_batch(gpu_lib)


def deflate_streams(lib, blocks):
    payload, cut = concat(blocks)
    cap = int(cut[-1]) + 5 * len(blocks) + 64
    out = np.zeros(cap, dtype=np.uint8)
    off = np.zeros(len(blocks) + 1, dtype=np.uint64)
    rc = lib.l.ssg_bgzf_deflate(payload.ctypes.data_as(C.c_void_p) if payload.size else None, cut.ctypes.data_as(C.c_void_p), C.c_long(len(blocks)),
                                out.ctypes.data_as(C.c_void_p), C.c_uint64(cap), off.ctypes.data_as(C.c_void_p))
    assert rc == 0, lib.l.ssg_last_error()
    return [out[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(blocks))]


def check_members(lib, blocks, want_crc=True):
    """every member of ssg_bgzf_compress(blocks) against gzip / zlib.crc32 and against ssg_bgzf_deflate's stream of the same input"""
    payload, cut = concat(blocks)
    out, off, crc = capi.bgzf_compress(lib, payload, cut, want_crc=want_crc)
    assert int(off[0]) == 0 and len(out) == int(off[-1]) <= capi.bgzf_bound(lib, len(payload), len(blocks)) == len(payload) + 31 * len(blocks)
    streams = deflate_streams(lib, blocks)
    whole = out.tobytes()
    for i, b in enumerate(blocks):
        m = whole[int(off[i]):int(off[i + 1])]
        assert m[:16] == HDR16 and struct.unpack("<H", m[16:18])[0] == len(m) - 1, (i, len(b), m[:18].hex())
        assert gzip.decompress(m) == b, (i, len(b))               # (checks the trailer's CRC-32 and ISIZE)
        assert struct.unpack("<II", m[-8:]) == (zlib.crc32(b), len(b)), (i, len(b))
        if want_crc:
            assert int(crc[i]) == zlib.crc32(b), (i, len(b))
        if b:
            assert m[18:-8] == streams[i], (i, len(b))
        else:
            assert m == EOF_MARKER, (i, m.hex())
    assert gzip.decompress(whole) == payload.tobytes()            # a multi-member gzip file
    return whole, off


@functools.lru_cache(maxsize=None)
def member_blocks():
    rng = np.random.RandomState(7)
    blocks = []
    for k, n in enumerate(BLOCK_LENGTHS):
        blocks += [text_shaped(rng, n), run_shaped(rng, n), rng.bytes(n), bam_shaped(n, k)]
    return blocks


def test_emu_bgzf_compress_members_are_valid_gzip(emu_lib):
    check_members(emu_lib, member_blocks())


@pytest.mark.gpu
def test_gpu_bgzf_compress_members_are_valid_gzip(gpu_lib):
    check_members(gpu_lib, member_blocks())


def check_empty_payloads(lib):
    x, y = b"not empty\n" * 30, bam_shaped(5000, 3)
    for blocks in ([b""], [b"", x], [x, b""], [x, b"", b"", y]):
        whole, off = check_members(lib, blocks)
        for i, b in enumerate(blocks):
            if not b:
                assert whole[int(off[i]):int(off[i + 1])] == EOF_MARKER
    assert check_members(lib, [b""])[0] == EOF_MARKER


def test_emu_bgzf_compress_empty_payload_is_the_eof_marker(emu_lib):
    check_empty_payloads(emu_lib)


@pytest.mark.gpu
def test_gpu_bgzf_compress_empty_payload_is_the_eof_marker(gpu_lib):
    check_empty_payloads(gpu_lib)


def check_edges(lib):
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    # no block: out_off[0] = 0, nothing else
    off = np.full(1, 77, dtype=np.uint64)
    out = np.full(64, 0xAB, dtype=np.uint8)
    assert lib.l.ssg_bgzf_compress(None, ptr(np.zeros(1, dtype=np.uint64)), C.c_long(0), ptr(out), C.c_uint64(0), ptr(off), None) == 0
    assert int(off[0]) == 0 and (out == 0xAB).all()
    # crc = NULL
    blocks = [bam_shaped(3000, 1), b"ab", run_shaped(np.random.RandomState(3), 700)]
    whole, moff = check_members(lib, blocks, want_crc=False)
    # a payload above 0xff00
    big, cut = concat([bytes(0xff01)])
    off = np.zeros(2, dtype=np.uint64)
    out = np.zeros(0xff01 + 64, dtype=np.uint8)
    assert lib.l.ssg_bgzf_compress(ptr(big), ptr(cut), C.c_long(1), ptr(out), C.c_uint64(out.size), ptr(off), None) == SSG_EINVAL
    assert b"0xff00" in lib.l.ssg_last_error()
    # out_cap one byte short: SSG_EOVERFLOW and nothing behind out + out_cap
    payload, cut = concat(blocks)
    cap = len(whole) - 1
    out = np.full(cap + 64, 0xAB, dtype=np.uint8)
    off = np.zeros(len(blocks) + 1, dtype=np.uint64)
    assert lib.l.ssg_bgzf_compress(ptr(payload), ptr(cut), C.c_long(len(blocks)), ptr(out), C.c_uint64(cap), ptr(off), None) == SSG_EOVERFLOW
    assert (out[cap:] == 0xAB).all()
    out = np.full(cap + 1 + 64, 0xAB, dtype=np.uint8)          # ... and the exact size is enough
    assert lib.l.ssg_bgzf_compress(ptr(payload), ptr(cut), C.c_long(len(blocks)), ptr(out), C.c_uint64(cap + 1), ptr(off), None) == 0
    assert out[:cap + 1].tobytes() == whole and (out[cap + 1:] == 0xAB).all()


def test_emu_bgzf_compress_edges(emu_lib):
    check_edges(emu_lib)


@pytest.mark.gpu
def test_gpu_bgzf_compress_edges(gpu_lib):
    check_edges(gpu_lib)


@functools.lru_cache(maxsize=None)
def batch_blocks():
    """4097 blocks: 4096 of three bytes and, behind them, one of the largest size -- the second device call's"""
    rng = np.random.RandomState(13)
    return [rng.bytes(3) for _ in range(4096)] + [bam_shaped(0xff00, 5)]


def test_emu_bgzf_compress_across_the_per_call_batch(emu_lib):
    check_members(emu_lib, batch_blocks())


@pytest.mark.gpu
def test_gpu_bgzf_compress_across_the_per_call_batch(gpu_lib):
    check_members(gpu_lib, batch_blocks())


def write_sam(path):
    """a few thousand records over three contigs, mates pointing at one another, unmapped reads among them and at the end"""
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


def check_sort(sambamba, tmp_path):
    d = str(tmp_path)
    write_sam(d + "/in.sam")
    with open(d + "/in.sam", "rb") as fi, open(d + "/u.bam", "wb") as fo:
        subprocess.run([sambamba, "view", "-S", "-f", "bam", "-l", "0", "/dev/stdin"], stdin=fi, stdout=fo, check=True)
    env = dict(os.environ, SSG_BGZF_DEVICE="1", SSG_SORT_DEV_BATCH="16", SSG_SORT_LOG="1")   # the device-deflate path, two batches for a small file
    env.pop("SSG_BGZF_DEVICE_CRC", None)
    files = {}
    for tag, extra, where in (("dev", {}, "device"), ("host", {"SSG_BGZF_DEVICE_CRC": "0"}, "host")):
        out = "%s/%s.bam" % (d, tag)
        r = subprocess.run([sambamba, "sort", "-t", "4", "-m", "1G", "--tmpdir=%s/tmp_%s" % (d, tag), "-o", out, d + "/u.bam"], check=True, capture_output=True, text=True, env=dict(env, **extra))
        assert int(re.search(r"write of (\d+) blocks", r.stderr).group(1)) > 16, r.stderr[-800:]      # more than one batch
        line = [l for l in r.stderr.split("\n") if "blocks deflated on" in l]
        assert len(line) == 1 and "CRC-32 on the %s" % where in line[0] and "CRC-32 on the %s" % {"device": "host", "host": "device"}[where] not in line[0], r.stderr[-800:]
        files[tag] = (open(out, "rb").read(), open(out + ".bai", "rb").read())
    assert files["dev"][0] == files["host"][0]                    # the same file, byte for byte, and the same index
    assert files["dev"][1] == files["host"][1]
    bam = files["dev"][0]
    assert bam.endswith(EOF_MARKER)
    plain = gzip.decompress(bam)                                  # every member's CRC-32 and ISIZE hold
    assert plain[:4] == b"BAM\1"
    # the records are all there, in coordinate order, the unplaced ones last
    l_text, = struct.unpack_from("<i", plain, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", plain, o); o += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", plain, o); o += 8 + l_name
    keys = []
    while o < len(plain):
        bs, tid, pos = struct.unpack_from("<iii", plain, o)
        keys.append((tid if tid >= 0 else 1 << 30, pos)); o += 4 + bs
    assert len(keys) == 6000 and keys == sorted(keys) and keys[-1][0] == 1 << 30 and keys[0][0] == 0


def test_emu_sambamba_sort_same_file_with_device_crc(tmp_path, emu_lib):
    check_sort(os.path.join(ROOT, "tests", "emu", "sambamba_emu"), tmp_path)


@pytest.mark.gpu
def test_gpu_sambamba_sort_same_file_with_device_crc(tmp_path, gpu_lib):
    check_sort(os.path.join(ROOT, "bin", "sambamba"), tmp_path)
