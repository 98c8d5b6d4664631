"""BAM read into the record store (k_bam_scan.h; ssg_recs_append_bgzf, ssg_recs_scan, ssg_recs_reopen, ssg_recs_release): members
inflated into a chunk and the chunk's records found on the device against a Python walk of the same bytes -- every field, every edge of the walk and of
the store's lifecycle -- and `sambamba merge' / `sambamba index' with SSG_MERGE_DEVICE=1 / SSG_INDEX_DEVICE=1 against their host paths: the same records,
the same index, every fall-back by its log line, and nothing new without the switches.  CPU-side on the host emulation of the kernels; `-m gpu' on the MI355X."""
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
from test_bgzf_inflate import concat, deflate, member

SSG_EIO, SSG_ENOMEM, SSG_EINVAL, SSG_EALIGN, SSG_EOVERFLOW = -5, -12, -22, -71, -75
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
M64 = (1 << 64) - 1
REF_CONSUMING = (0, 2, 3, 7, 8)   # M D N = X


def rec(tid=0, pos=0, flag=0, cigar=(), name=b"r\0", l_seq=0, extra=b"", block_size=None):
    """one BAM record: block_size word and body; block_size (if given) is reached by padding the tags"""
    cig = b"".join(struct.pack("<I", n << 4 | op) for n, op in cigar)
    body = (struct.pack("<iiIIiiii", tid, pos, len(name) | 30 << 8 | 4681 << 16, (flag << 16) | len(cigar), l_seq, -1, -1, 0) + name + cig
            + bytes((l_seq + 1) // 2) + bytes([30]) * l_seq + extra)
    if block_size is not None:
        assert block_size >= len(body)
        body += bytes(block_size - len(body))
    return struct.pack("<I", len(body)) + body


def py_walk(stream, first, chunk):
    """the reference: loc, key, ent of every record of stream[first:]"""
    loc, key, ent, o = [], [], [], first
    while o < len(stream):
        bs, tid, pos, bmn, fnc = struct.unpack_from("<IiiII", stream, o)
        assert bs >= 32 and o + 4 + bs <= len(stream)
        l_qname, flag, nc = bmn & 0xff, fnc >> 16, fnc & 0xffff
        end = pos + 1
        if not (flag & 4) and nc:
            ops = struct.unpack_from("<%dI" % nc, stream, o + 36 + l_qname)
            end = pos + sum(v >> 4 for v in ops if (v & 0xf) in REF_CONSUMING)
        loc.append(chunk << 40 | o)
        key.append(((tid << 32) & M64) | (((pos + 1) << 1) & 0xffffffff) | (1 if flag & 0x10 else 0))
        ent.append((tid, pos, end, flag, 4 + bs, 0))
        o += 4 + bs
    return np.array(loc, dtype=np.uint64), np.array(key, dtype=np.uint64), np.array(ent, dtype=capi.BAM_ENT_DT)


def make_member(payload, kind):
    if kind == "stored":
        return member(deflate(payload, 0), payload)
    if kind == "fixed":
        return member(deflate(payload, 6, strategy=zlib.Z_FIXED), payload)
    return member(deflate(payload, 6), payload)


KINDS = ("stored", "fixed", "dynamic")


def small_members(n, seed):
    """n members of two or three tiny records with random fields"""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        recs = []
        for _ in range(int(rng.randint(2, 4))):
            ops = [(int(rng.randint(1, 60)), int(rng.randint(0, 9))) for _ in range(int(rng.randint(0, 4)))]
            recs.append(rec(int(rng.randint(-1, 5)), int(rng.randint(-1, 1 << 20)), int(rng.choice([0, 4, 16, 20, 99, 147])), ops,
                            name=b"q%d\0" % rng.randint(1000), l_seq=int(rng.randint(0, 9)), extra=bytes(rng.randint(0, 7))))
        out.append(b"".join(recs))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (payload of every member, first)"""
    c = {}
    for n in (1, 63, 64, 65, 4097):
        c["members_%d" % n] = (small_members(n, 100 + n), 0)
    p = small_members(9, 7)
    c["empty_members"] = (p[:4] + [b""] + p[4:] + [b""], 0)
    hdr = b"BAM\1" + struct.pack("<i", 13) + b"@HD\tVN:1.3\n\0\0" + struct.pack("<i", 1) + struct.pack("<i", 5) + b"ctgA\0" + struct.pack("<i", 400000)
    c["first"] = ([hdr + p[0]] + p[1:4], len(hdr))
    c["first_whole_member"] = ([hdr] + p[1:4], len(hdr))
    c["block_size_32"] = ([rec(name=b"", block_size=32)], 0)
    c["full_member"] = ([p[0], rec(2, 77, 0, [(50, 0)], block_size=0xff00 - 4), p[1]], 0)
    every_op = [(3 + k, k) for k in range(9)]
    c["fields"] = ([rec(1, 100, 0, []) + rec(1, 200, 4, [(40, 0), (2, 2), (10, 0)]) + rec(1, 300, 0, every_op),
                    rec(1, 400, 16, [(1 + k % 7, k % 9) for k in range(1000)]) + rec(1, (1 << 29) - 1, 0, [(100, 0)]),
                    rec(-1, -1, 4 | 64, []) + rec(-1, -1, 4 | 16 | 128, [])], 0)
    return c


def kinds_of(n):
    return [KINDS[k % 3] for k in range(n)]


def load(lib, payloads, cap=1 << 40):
    members = [make_member(p, k) for p, k in zip(payloads, kinds_of(len(payloads)))]
    blob, moff = concat(members)
    recs = capi.recs_create(lib, cap)
    rc, cid, off, st = capi.recs_append_bgzf(lib, recs, blob, moff)
    assert rc == 0 and cid == 0 and (st == 0).all(), lib.l.ssg_last_error()
    want = np.zeros(len(payloads) + 1, dtype=np.uint64)
    want[1:] = np.cumsum([len(p) for p in payloads])
    assert (off == want).all()
    return recs, cid, off


def same(got, want):
    n, loc, key, ent = got
    wloc, wkey, went = want
    assert n == len(wloc)
    assert (loc == wloc).all() and (key == wkey).all()
    for f in capi.BAM_ENT_DT.names:
        assert (ent[f] == went[f]).all(), f


def check_case(lib, name):
    payloads, first = cases()[name]
    if name.startswith("members_"):
        assert len(payloads) == int(name.split("_")[1])
    recs, cid, off = load(lib, payloads)
    stream = b"".join(payloads)
    want = py_walk(stream, first, cid)
    assert len(want[0]) >= 1
    rc, n, loc, key, ent = capi.recs_scan(lib, recs, cid, off, first)
    assert rc == 0, lib.l.ssg_last_error()
    same((n, loc, key, ent), want)
    # the payload is what the members hold: the records gathered in stream order are the stream
    cum = np.concatenate([[0], np.cumsum(ent["len"].astype(np.uint64))]).astype(np.uint64)
    capi.recs_order(lib, recs, loc, cum)
    assert capi.recs_gather(lib, recs, 0, int(cum[-1])).tobytes() == stream[first:]
    recs.close()


CASES = ["members_1", "members_63", "members_64", "members_65", "members_4097", "empty_members", "first", "first_whole_member", "block_size_32", "full_member", "fields"]


@pytest.mark.parametrize("name", CASES)
def test_emu_scan_equals_python_walk(emu_lib, name):
    check_case(emu_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_gpu_scan_equals_python_walk(gpu_lib, name):
    check_case(gpu_lib, name)


def test_the_cases_are_what_they_are_meant_to_be():
    c = cases()
    assert sorted(c) == sorted(CASES)
    loc, key, ent = py_walk(b"".join(c["fields"][0]), 0, 0)
    assert list(ent["end"][:4]) == [101, 201, 300 + sum(3 + k for k in REF_CONSUMING), 400 + sum(1 + k % 7 for k in range(1000) if k % 9 in REF_CONSUMING)]
    assert int(key[-1]) == 0xffffffff00000001 and int(key[-2]) == 0xffffffff00000000 and int(key[4]) == 1 << 32 | 1 << 30
    assert len(c["full_member"][0][1]) == 0xff00 and len(c["block_size_32"][0][0]) == 36
    assert set(kinds_of(5)) == set(KINDS)


def check_misaligned(lib):
    p = small_members(4, 31)
    stream = b"".join(p)
    a, b = len(p[0]), len(p[0]) + len(p[1]) + len(p[2]) - 11             # the third record group is cut 11 bytes before its end: member 2 begins inside a record
    payloads = [stream[:a], stream[a:b], stream[b:]]
    recs, cid, off = load(lib, payloads, cap=len(stream))
    rc, n, loc, key, ent = capi.recs_scan(lib, recs, cid, off, 0)
    assert rc == SSG_EALIGN and re.search(rb"not record-aligned at hint 1\b", lib.l.ssg_last_error()), lib.l.ssg_last_error()
    assert (loc == 0xABABABABABABABAB).all() and (key == 0xABABABABABABABAB).all() and ent.tobytes() == b"\xab" * ent.nbytes   # nothing returned as valid
    # the store is unchanged and usable: the same chunk with the one hint that holds is the whole stream
    rc, n, loc, key, ent = capi.recs_scan(lib, recs, cid, [0, len(stream)], 0)
    assert rc == 0
    same((n, loc, key, ent), py_walk(stream, 0, cid))
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    one = np.zeros(1, dtype=np.uint8)
    assert lib.l.ssg_recs_append(recs.h, ptr(one), C.c_uint64(1), None) == SSG_ENOMEM                  # (the capacity is exactly the chunk's)
    recs.close()


def test_emu_scan_reports_a_record_cut_across_members(emu_lib):
    check_misaligned(emu_lib)


@pytest.mark.gpu
def test_gpu_scan_reports_a_record_cut_across_members(gpu_lib):
    check_misaligned(gpu_lib)


def check_malformed(lib):
    p = small_members(6, 37)
    good = b"".join(p)
    at = len(p[0]) + len(p[1])                                            # the first record of member 2

    def scan(stream, cuts):
        recs, cid, off = load(lib, [stream[a:b] for a, b in zip(cuts[:-1], cuts[1:])])
        rc, n, loc, key, ent = capi.recs_scan(lib, recs, cid, off, 0)
        msg = lib.l.ssg_last_error()
        recs.close()
        return rc, msg
    cuts = [0] + list(np.cumsum([len(x) for x in p]))
    # block_size 31
    bad = bytearray(good); struct.pack_into("<I", bad, at, 31)
    rc, msg = scan(bytes(bad), cuts)
    assert rc == SSG_EIO and b"offset %d" % at in msg and b"below 32" in msg, msg
    # a block_size that runs past the chunk's end (the last record's), and one that is all ones
    loc, _, _ = py_walk(good, 0, 0)
    last = int(loc[-1])
    for v in (len(good) - last - 4 + 1, 0xffffffff):
        bad = bytearray(good); struct.pack_into("<I", bad, last, v)
        rc, msg = scan(bytes(bad), cuts)
        assert rc == SSG_EIO and b"offset %d" % last in msg and b"past the end" in msg, msg
    # fewer than four bytes behind the last record
    rc, msg = scan(good + b"\x24\x00", cuts[:-1] + [len(good) + 2])
    assert rc == SSG_EIO and b"offset %d" % len(good) in msg, msg
    # l_qname + 4 n_cigar past the record
    bs, = struct.unpack_from("<I", good, at)
    bad = bytearray(good); struct.pack_into("<I", bad, at + 16, (bs // 4) + 1)   # flag 0, n_cigar = block_size / 4 + 1
    rc, msg = scan(bytes(bad), cuts)
    assert rc == SSG_EIO and b"offset %d" % at in msg and b"n_cigar" in msg, msg


def test_emu_scan_refuses_malformed_streams(emu_lib):
    check_malformed(emu_lib)


@pytest.mark.gpu
def test_gpu_scan_refuses_malformed_streams(gpu_lib):
    check_malformed(gpu_lib)


def check_cap_and_crc(lib):
    p = small_members(5, 41)
    stream = b"".join(p)
    want = py_walk(stream, 0, 0)
    n_want = len(want[0])
    # cap one too small
    recs, cid, off = load(lib, p, cap=len(stream))
    rc, n, loc, key, ent = capi.recs_scan(lib, recs, cid, off, 0, cap=n_want - 1)
    assert rc == SSG_EOVERFLOW and n == n_want
    assert (loc == 0xABABABABABABABAB).all() and (key == 0xABABABABABABABAB).all() and ent.tobytes() == b"\xab" * ent.nbytes   # (the element behind cap among them)
    rc, n, loc, key, ent = capi.recs_scan(lib, recs, cid, off, 0, cap=n_want)
    assert rc == 0
    same((n, loc, key, ent), want)
    recs.close()
    # a member with a wrong CRC: status as ssg_bgzf_inflate gives it, no chunk, the capacity unchanged
    members = [make_member(x, k) for x, k in zip(p, kinds_of(len(p)))]
    broken = list(members)
    broken[3] = members[3][:-8] + struct.pack("<I", struct.unpack("<I", members[3][-8:-4])[0] ^ 1) + members[3][-4:]
    recs = capi.recs_create(lib, len(stream))
    blob, moff = concat(broken)
    rc, cid, off, st = capi.recs_append_bgzf(lib, recs, blob, moff)
    rc2, _, off2, st2 = capi.bgzf_inflate(lib, blob, moff)
    assert rc == SSG_EIO and rc2 == SSG_EIO and cid is None and list(st) == [0, 0, 0, 3, 0] and list(st2) == list(st) and (off == off2).all()
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    n_rec = C.c_uint64(7)
    hint = np.array([0, 1], dtype=np.uint64)
    assert lib.l.ssg_recs_scan(recs.h, C.c_uint32(0), ptr(hint), C.c_int64(1), C.c_uint64(0), C.c_uint64(0), C.byref(n_rec), None, None, None) == SSG_EINVAL   # no chunk 0
    blob, moff = concat(members)
    rc, cid, off, st = capi.recs_append_bgzf(lib, recs, blob, moff)                                    # all of the capacity is still there, and the id
    assert rc == 0 and cid == 0
    rc, n, loc, key, ent = capi.recs_scan(lib, recs, cid, off, 0)
    same((n, loc, key, ent), want)
    # what ssg_bgzf_inflate refuses by the header is refused here, and leaves the store as it was
    short = np.frombuffer(members[0][:27], dtype=np.uint8)
    o = np.zeros(2, dtype=np.uint64)
    assert lib.l.ssg_recs_append_bgzf(recs.h, ptr(short), ptr(np.array([0, 27], dtype=np.uint64)), C.c_long(1), None, ptr(o), None) == SSG_EINVAL
    assert b"member 0" in lib.l.ssg_last_error()
    assert lib.l.ssg_recs_append_bgzf(recs.h, ptr(blob), ptr(moff), C.c_long(len(members)), None, ptr(off), None) == SSG_ENOMEM
    assert b"capacity" in lib.l.ssg_last_error()
    rc, n, loc, key, ent = capi.recs_scan(lib, recs, 0, off, 0)
    same((n, loc, key, ent), want)
    recs.close()


def test_emu_scan_cap_and_a_bad_member(emu_lib):
    check_cap_and_crc(emu_lib)


@pytest.mark.gpu
def test_gpu_scan_cap_and_a_bad_member(gpu_lib):
    check_cap_and_crc(gpu_lib)


def check_lifecycle(lib):
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    pa, pb, pc = small_members(3, 43), small_members(4, 47), small_members(2, 53)
    sa, sb, sc = b"".join(pa), b"".join(pb), b"".join(pc)
    recs = capi.recs_create(lib, len(sa) + len(sb) + len(sc))
    chunks = []
    for p in (pa, pb):
        blob, moff = concat([make_member(x, k) for x, k in zip(p, kinds_of(len(p)))])
        rc, cid, off, _ = capi.recs_append_bgzf(lib, recs, blob, moff)
        rc2, n, loc, key, ent = capi.recs_scan(lib, recs, cid, off, 0)
        assert rc == 0 and rc2 == 0 and cid == len(chunks)
        chunks.append((loc, ent["len"].astype(np.uint64)))

    def order_and_gather(parts, streams, seed):
        loc = np.concatenate([x[0] for x in parts]); ln = np.concatenate([x[1] for x in parts])
        perm = np.random.RandomState(seed).permutation(len(loc))
        cum = np.concatenate([[0], np.cumsum(ln[perm])]).astype(np.uint64)
        capi.recs_order(lib, recs, loc[perm], cum)
        want = b"".join(streams[int(l) >> 40][int(l) & ((1 << 40) - 1):][:int(k)] for l, k in zip(loc[perm], ln[perm]))
        assert capi.recs_gather(lib, recs, 0, int(cum[-1])).tobytes() == want
    order_and_gather(chunks, [sa, sb], 1)
    # an order is declared: no append of either kind, no release
    c_arr = np.frombuffer(sc, dtype=np.uint8)
    blob_c, moff_c = concat([make_member(x, "dynamic") for x in pc])
    o = np.zeros(len(pc) + 1, dtype=np.uint64)
    assert lib.l.ssg_recs_append(recs.h, ptr(c_arr), C.c_uint64(c_arr.size), None) == SSG_EINVAL
    assert lib.l.ssg_recs_append_bgzf(recs.h, ptr(blob_c), ptr(moff_c), C.c_long(len(pc)), None, ptr(o), None) == SSG_EINVAL
    assert lib.l.ssg_recs_release(recs.h, C.c_uint32(0)) == SSG_EINVAL and b"reopen" in lib.l.ssg_last_error()
    # reopen, append, a second order gathers the new stream
    capi.recs_reopen(lib, recs)
    rc, cid, off, _ = capi.recs_append_bgzf(lib, recs, blob_c, moff_c)
    rc2, n, loc, key, ent = capi.recs_scan(lib, recs, cid, off, 0)
    assert rc == 0 and rc2 == 0 and cid == 2
    chunks.append((loc, ent["len"].astype(np.uint64)))
    order_and_gather(chunks, [sa, sb, sc], 2)
    # release: the capacity comes back, the id stays taken, an order that names the chunk is refused
    capi.recs_reopen(lib, recs)
    one = np.zeros(1, dtype=np.uint8)
    assert lib.l.ssg_recs_append(recs.h, ptr(one), C.c_uint64(1), None) == SSG_ENOMEM                  # full
    capi.recs_release(lib, recs, 0)
    assert lib.l.ssg_recs_release(recs.h, C.c_uint32(0)) == SSG_EINVAL                                 # once
    assert lib.l.ssg_recs_release(recs.h, C.c_uint32(3)) == SSG_EINVAL                                 # no such chunk
    a_arr = np.frombuffer(sa, dtype=np.uint8)
    assert capi.recs_append(lib, recs, a_arr) == 3                                                     # exactly chunk 0's bytes fit again
    assert lib.l.ssg_recs_append(recs.h, ptr(one), C.c_uint64(1), None) == SSG_ENOMEM
    l0, c0 = np.array([0], dtype=np.uint64), np.array([0, 0], dtype=np.uint64)
    assert lib.l.ssg_recs_order(recs.h, ptr(l0), ptr(c0), C.c_int64(1)) == SSG_EINVAL and b"released" in lib.l.ssg_last_error()
    assert lib.l.ssg_recs_order(recs.h, ptr(chunks[0][0]), ptr(np.concatenate([[0], np.cumsum(chunks[0][1])]).astype(np.uint64)), C.c_int64(len(chunks[0][0]))) == SSG_EINVAL
    n_rec = C.c_uint64(0)
    assert lib.l.ssg_recs_scan(recs.h, C.c_uint32(0), ptr(np.array([0, 1], dtype=np.uint64)), C.c_int64(1), C.c_uint64(0), C.c_uint64(0), C.byref(n_rec), None, None, None) == SSG_EINVAL
    moved = (chunks[0][0] & np.uint64((1 << 40) - 1)) | np.uint64(3 << 40)
    order_and_gather([chunks[1], chunks[2], (moved, chunks[0][1])], [None, sb, sc, sa], 3)             # the others are where they were
    recs.close()


def test_emu_store_reopen_and_release(emu_lib):
    check_lifecycle(emu_lib)


@pytest.mark.gpu
def test_gpu_store_reopen_and_release(gpu_lib):
    check_lifecycle(gpu_lib)


def test_emu_device_memory(emu_lib):
    free, total = capi.device_memory(emu_lib)
    assert 0 < free <= total


@pytest.mark.gpu
def test_gpu_device_memory(gpu_lib):
    free, total = capi.device_memory(gpu_lib)
    assert (1 << 30) < free <= total                                                  # (what the merge sizes its window from)


# ---------------- sambamba merge / index ----------------
CTG = [("ctgA", 400000), ("ctgB", 250000), ("ctgC", 90000)]
OURS = ("SSG_MERGE_DEVICE", "SSG_MERGE_WINDOW", "SSG_MERGE_POOL", "SSG_INDEX_DEVICE", "SSG_BGZF_INFLATE_DEVICE", "SSG_BGZF_DEVICE", "SSG_DEBUG", "SSG_SORT_LOG", "SSG_BAM_LEVEL",
        "SSG_SORT_DEVICE_GATHER", "HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES")


def write_sam(path, seed, n, tail, shared, rg):
    """n mapped records at random places, `shared' places that every input has (so that input order decides), `tail' unmapped records at the end"""
    rng = np.random.RandomState(seed)
    with open(path, "w") as f:
        f.write("@HD\tVN:1.3\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CTG) + "@RG\tID:%s\tSM:s\n" % rg)
        def line(name, flag, ctg, pos, cigar):
            seq = "".join("ACGT"[b] for b in rng.randint(0, 4, size=100)); qual = "".join(chr(33 + q) for q in rng.choice([40, 40, 37, 12], size=100))
            f.write("%s\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t%s\tRG:Z:%s\n" % (name, flag, ctg, pos, 60 if ctg != "*" else 0, cigar, seq, qual, rg))
        for i in range(n):
            name, ln = CTG[rng.randint(3)]
            line("%s_m%d" % (rg, i), int(rng.choice([0, 16])), name, int(rng.randint(1, ln - 200)), str(rng.choice(["100M", "60M2D40M", "30S70M", "50M1000N50M"])))
        for k, (c, p, fl) in enumerate(shared):
            for j in range(3):
                line("%s_s%d_%d" % (rg, k, j), fl, c, p, "100M")
        for i in range(tail):
            line("%s_u%d" % (rg, i), 4, "*", 0, "*")


def payload_of(bam):
    return gzip.decompress(bam)


def members_of(bam):
    out, o = [], 0
    while o < len(bam):
        bsize = struct.unpack_from("<H", bam, o + 16)[0] + 1
        out.append(bam[o:o + bsize]); o += bsize
    return out


def reblock(bam, step=None, header_shares=False):
    """the same BAM with other blocks: cut every `step' bytes whatever lies there, or (header_shares) at records with the header and the first records in one block"""
    plain = payload_of(bam)
    l_text, = struct.unpack_from("<i", plain, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", plain, o); o += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", plain, o); o += 8 + l_name
    if step:
        cuts = list(range(0, len(plain), step)) + [len(plain)]
    else:
        cuts, last = [0], 0
        while o < len(plain):
            bs, = struct.unpack_from("<I", plain, o)
            if o + 4 + bs - last > 20000 and o > last and (last > 0 or not header_shares or o > 8 + l_text + 3000):
                cuts.append(o); last = o
            o += 4 + bs
        cuts.append(len(plain))
    return b"".join(make_member(plain[a:b], "dynamic") for a, b in zip(cuts[:-1], cuts[1:])) + EOF_MARKER


SHARED = [("ctgA", 1000, 0), ("ctgA", 1000, 16), ("ctgB", 77, 0), ("ctgC", 89000, 16)]


class Merger:
    """the inputs of a session, made through the product's own view and sort, and every run of merge / index on them under another environment"""

    def __init__(self, sambamba, d):
        self.sambamba, self.d, self.runs = sambamba, str(d), {}
        self.clean = {k: v for k, v in os.environ.items() if k not in OURS}
        for name, seed, n, tail, rg in (("a", 1, 1500, 700, "ga"), ("b", 2, 1200, 300, "gb"), ("c", 3, 600, 50, "gc")):
            write_sam("%s/%s.sam" % (self.d, name), seed, n, tail, SHARED, rg)
            self.view("%s/%s.sam" % (self.d, name), "%s/%s.u.bam" % (self.d, name))
            subprocess.run([sambamba, "sort", "-t", "4", "-m", "1G", "--tmpdir=%s/tmp_%s" % (self.d, name), "-o", "%s/%s.bam" % (self.d, name), "%s/%s.u.bam" % (self.d, name)],
                           check=True, capture_output=True, env=self.clean)
        with open(self.d + "/empty.sam", "w") as f:
            f.write("@HD\tVN:1.3\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CTG) + "@RG\tID:ge\tSM:s\n")
        self.view(self.d + "/empty.sam", self.d + "/empty.bam")
        open(self.d + "/skew.bam", "wb").write(reblock(open(self.d + "/b.bam", "rb").read(), step=30011))

    def view(self, sam, bam):
        with open(sam, "rb") as fi, open(bam, "wb") as fo:
            subprocess.run([self.sambamba, "view", "-S", "-f", "bam", "/dev/stdin"], stdin=fi, stdout=fo, check=True, env=self.clean)

    def path(self, name):
        return "%s/%s.bam" % (self.d, name)

    def merge(self, tag, inputs, extra, args=(), check=True):
        if tag not in self.runs:
            env = dict(self.clean, SSG_DEBUG="1"); env.update(extra)
            out = "%s/out_%s.bam" % (self.d, tag)
            r = subprocess.run([self.sambamba, "merge", "-t", "4"] + list(args) + [out] + [self.path(x) for x in inputs], capture_output=True, text=True, env=env)
            if check:
                assert r.returncode == 0, r.stderr[-2000:]
            self.runs[tag] = (out, r)
        return self.runs[tag]

    def index(self, bam, extra):
        """the .bai `sambamba index' writes for a copy of the file (no note of a writer next to it), and the log"""
        tmp = "%s/ix_%d.bam" % (self.d, len(os.listdir(self.d)))
        open(tmp, "wb").write(open(bam, "rb").read())
        env = dict(self.clean, SSG_DEBUG="1"); env.update(extra)
        r = subprocess.run([self.sambamba, "index", "-t", "4", tmp], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(tmp + ".bai", "rb").read(), r.stderr


@pytest.fixture(scope="module")
def emu_merger(tmp_path_factory, emu_lib):
    return Merger(os.path.join(ROOT, "tests", "emu", "sambamba_emu"), tmp_path_factory.mktemp("bam_scan_emu"))


@pytest.fixture(scope="module")
def gpu_merger(tmp_path_factory, gpu_lib):
    return Merger(os.path.join(ROOT, "bin", "sambamba"), tmp_path_factory.mktemp("bam_scan_gpu"))


DEV = {"SSG_MERGE_DEVICE": "1"}
# inputs, SSG_MERGE_WINDOW (None: the default), what the log must say about the rounds
MERGES = {
    "two": (("a", "b"), None, lambda rounds: rounds == 1),                      # larger than the inputs: one round
    "three": (("a", "b", "c"), "1", lambda rounds: rounds > 8),                  # one member per input and round
    "tail": (("b", "a", "c"), "100000", lambda rounds: rounds > 2),              # smaller than the 700 unmapped records of one key at the end of a
    "with_empty": (("a", "empty", "b"), "150000", lambda rounds: rounds > 1),    # an input that is a header only
    "only_empty": (("empty", "empty"), None, lambda rounds: rounds == 0),
}


def check_merge(m, name):
    inputs, window, rounds_ok = MERGES[name]
    host_out, _ = m.merge("host_" + name, inputs, {})
    dev_out, r = m.merge("dev_" + name, inputs, dict(DEV, **({"SSG_MERGE_WINDOW": window} if window else {})))
    host, dev = open(host_out, "rb").read(), open(dev_out, "rb").read()
    assert payload_of(dev) == payload_of(host)                                       # the same records in the same order under the same header
    assert dev.endswith(EOF_MARKER)
    line = [l for l in r.stderr.split("\n") if "merged on the device" in l]
    assert len(line) == 1 and "device merge off" not in r.stderr, r.stderr[-2000:]
    assert rounds_ok(int(re.search(r"in (\d+) round", line[0]).group(1))), line[0]
    # the index written with the file is the one the host `sambamba index' makes of it, and the note says so
    want_bai, _ = m.index(dev_out, {})
    assert open(dev_out + ".bai", "rb").read() == want_bai
    assert os.path.exists(dev_out + ".bai.ssg")
    env = dict(m.clean, SSG_DEBUG="1")
    r2 = subprocess.run([m.sambamba, "index", dev_out], capture_output=True, text=True, env=env)
    assert r2.returncode == 0 and "written by the sort is current" in r2.stderr, r2.stderr
    if name == "three":
        # keys that the inputs share: input order decided
        plain = payload_of(dev)
        for k in range(len(SHARED)):
            at = [plain.find(b"%s_s%d_0\0" % (g, k)) for g in (b"ga", b"gb", b"gc")]
            assert -1 not in at and at == sorted(at), (k, at)


@pytest.mark.parametrize("name", sorted(MERGES))
def test_emu_sambamba_merge_device_writes_the_same_records(emu_merger, name):
    check_merge(emu_merger, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MERGES))
def test_gpu_sambamba_merge_device_writes_the_same_records(gpu_merger, name):
    check_merge(gpu_merger, name)


# what turns the device merge off: inputs, environment, arguments, the reason in the one log line
FALLBACKS = {
    "level0": (("a", "b"), {}, ("-l", "0"), r"device merge off \(-l 0"),
    "skew": (("a", "skew"), {}, (), r"device merge off \(.*skew\.bam is not record-aligned at hint \d+"),
    "pool": (("a", "b"), {"SSG_MERGE_POOL": "100000"}, (), r"device merge off \(.*capacity"),
    "nodev": (("a", "b"), {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}, (), r"device merge off \(no device"),   # (the emulation always has a device)
}


def check_merge_fallback(m, name):
    inputs, extra, args, reason = FALLBACKS[name]
    host_out, _ = m.merge("fbhost_" + name, inputs, {}, args)
    out, r = m.merge("fb_" + name, inputs, dict(DEV, **extra), args)
    assert len([l for l in r.stderr.split("\n") if re.search(reason, l)]) == 1, r.stderr[-2000:]
    assert "merged on the device" not in r.stderr
    assert open(out, "rb").read() == open(host_out, "rb").read()                     # the host path's file, byte for byte
    assert not os.path.exists(out + ".bai")


@pytest.mark.parametrize("name", ["level0", "skew", "pool"])
def test_emu_sambamba_merge_fallbacks_write_the_host_file(emu_merger, name):
    check_merge_fallback(emu_merger, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_gpu_sambamba_merge_fallbacks_write_the_host_file(gpu_merger, name):
    check_merge_fallback(gpu_merger, name)


def check_merge_refusals_and_default(m):
    # an input that descends: refused with the file and the record (the host path merges it silently, and the device path would index it)
    open(m.path("desc"), "wb").write(reblock(open(m.path("b.u"), "rb").read()))      # (the records as they came, in blocks that start at records)
    out, r = m.merge("descends", ("a", "desc"), DEV, check=False)
    assert r.returncode != 0 and re.search(r"desc\.bam is not coordinate-sorted: its record \d+ ", r.stderr), r.stderr[-2000:]
    assert not os.path.exists(out)
    # a later round that is not record-aligned: the command ends, names the switch, removes what it wrote
    skew_late = m.path("skew_late")
    good = open(m.path("b"), "rb").read()
    ms = members_of(good)
    plain_tail = b"".join(payload_of(x) for x in ms[3:-1])
    open(skew_late, "wb").write(b"".join(ms[:3]) + b"".join(make_member(plain_tail[a:a + 30011], "dynamic") for a in range(0, len(plain_tail), 30011)) + EOF_MARKER)
    assert payload_of(open(skew_late, "rb").read()) == payload_of(good)
    out, r = m.merge("skew_late", ("a", "skew_late"), dict(DEV, SSG_MERGE_WINDOW="140000"), check=False)   # (two members of the sort a load)
    assert r.returncode != 0 and "SSG_MERGE_DEVICE=0" in r.stderr and "not record-aligned" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(out)
    # without the switch: today's log (none) and today's file
    out0, r0 = m.merge("unset", ("a", "b"), {})
    out1, r1 = m.merge("zero", ("a", "b"), {"SSG_MERGE_DEVICE": "0"})
    assert [l for l in (r0.stderr + r1.stderr).split("\n") if l.startswith("[sambamba] merge")] == []
    assert open(out0, "rb").read() == open(out1, "rb").read() and not os.path.exists(out0 + ".bai")


def test_emu_sambamba_merge_refusals_and_default(emu_merger):
    check_merge_refusals_and_default(emu_merger)


@pytest.mark.gpu
def test_gpu_sambamba_merge_refusals_and_default(gpu_merger):
    check_merge_refusals_and_default(gpu_merger)


def check_index(m):
    merged, _ = m.merge("host_three", ("a", "b", "c"), {})                          # 3300 mapped records over three contigs, 1050 unmapped at the end
    files = {"sorted": merged, "shared": m.d + "/shared.bam", "unaligned": m.d + "/unaligned.bam"}
    bam = open(merged, "rb").read()
    open(files["shared"], "wb").write(reblock(bam, header_shares=True))
    open(files["unaligned"], "wb").write(reblock(bam, step=50021))
    first = payload_of(members_of(open(files["shared"], "rb").read())[0])
    assert first[:4] == b"BAM\1" and b"ga_" in first                                 # the header shares its block with records
    for name, path in files.items():
        host, hlog = m.index(path, {})
        dev, dlog = m.index(path, {"SSG_INDEX_DEVICE": "1"})
        assert dev == host and len(host) > 500, name
        assert "device" not in hlog
        if name == "unaligned":
            assert len(re.findall(r"device index off \(.*not record-aligned at hint \d+", dlog)) == 1 and "found on the device" not in dlog, dlog
        else:
            assert "device index off" not in dlog and len(re.findall(r"index: (\d+) records found on the device", dlog)) == 1, dlog
            assert int(re.search(r"index: (\d+) records found", dlog).group(1)) == 4350 + 3 * 3 * len(SHARED)


def test_emu_sambamba_index_device_writes_the_same_index(emu_merger):
    check_index(emu_merger)


@pytest.mark.gpu
def test_gpu_sambamba_index_device_writes_the_same_index(gpu_merger):
    check_index(gpu_merger)
