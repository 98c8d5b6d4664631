"""BGZF inflate on the device (k_bgzf_inflate.h; ssg_bgzf_inflate, the inverse of ssg_bgzf_compress) against Python's zlib and
nothing else: members of every block type from zlib.compressobj and from this library's own deflate, hand-made fixed-Huffman streams zlib never
emits (distances up to 32768, matches whose source the step before wrote), malformed members (each one first shown to be refused by zlib; the
error paths must return and touch nothing outside the member's range), the edges of the entry point, the per-call batch, and sambamba's readers
with the device hook on and off.  CPU-side on the host emulation of the kernel; `-m gpu` on the MI355X."""
import ctypes as C
import functools
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from common import ROOT
from speedseq_amd import capi
from test_bgzf_frame import BLOCK_LENGTHS, EOF_MARKER, LENGTHS, bam_shaped, run_shaped, text_shaped, write_sam

SSG_EIO, SSG_EINVAL, SSG_EOVERFLOW = -5, -22, -75
assert 0 in BLOCK_LENGTHS and 0xff00 in BLOCK_LENGTHS and max(LENGTHS) > 0xff00


def frame(stream, crc, isize, pad=0):
    """a BGZF member around a deflate stream; pad > 0: one more subfield of that many bytes in front of BC"""
    extra = (b"XY" + struct.pack("<H", pad - 4) + bytes(pad - 4) if pad else b"")
    total = 12 + len(extra) + 6 + len(stream) + 8
    assert total <= 65536, total
    extra += b"BC" + struct.pack("<HH", 2, total - 1)
    return bytes.fromhex("1f8b08040000000000ff") + struct.pack("<H", len(extra)) + extra + stream + struct.pack("<II", crc, isize)


def member(stream, payload, pad=0):
    return frame(stream, zlib.crc32(payload), len(payload), pad)


def deflate(payload, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    return c.compress(payload) + c.flush()


def zlib_verdict(m):
    """the rule of the tests: what zlib makes of the member's stream, and whether the member is good"""
    xlen, = struct.unpack_from("<H", m, 10)
    s = m[12 + xlen:-8]
    crc, isize = struct.unpack("<II", m[-8:])
    d = zlib.decompressobj(-15)
    try:
        o = d.decompress(s, isize + 1)
    except zlib.error:
        return False, None
    return bool(d.eof and len(o) == isize and zlib.crc32(o) == crc), o


def concat(members):
    off = np.zeros(len(members) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in members])
    return np.frombuffer(b"".join(members), dtype=np.uint8), off


def call(lib, members, want_status=True, cap=None, guard=64):
    """ssg_bgzf_inflate with `guard` bytes of 0xAB behind out_cap: (rc, out[:out_off[-1]], out_off, status); the guard is checked here"""
    blob, moff = concat(members)
    n = len(members)
    need = sum(struct.unpack("<I", m[-4:])[0] for m in members)
    cap = need if cap is None else cap
    out = np.full(cap + guard, 0xAB, dtype=np.uint8)
    off = np.full(n + 1, 77, dtype=np.uint64)
    st = np.full(max(n, 1), -9, dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.l.ssg_bgzf_inflate(ptr(blob) if blob.size else None, ptr(moff), C.c_long(n), ptr(out), C.c_uint64(cap), ptr(off), ptr(st) if want_status else None)
    assert (out[cap:] == 0xAB).all(), "bytes behind out + out_cap were written"
    return rc, out[:min(int(off[n]), cap)] if rc in (0, SSG_EIO) else out[:cap], off, st[:n]


def check_good(lib, members, payloads, every_alignment=False):
    for m, p in zip(members, payloads):
        ok, o = zlib_verdict(m)
        assert ok and o == p, (len(p), m[:24].hex())                     # the fixture is what it is meant to be
    if every_alignment:
        _, moff = concat(members)
        assert set(int(x) % 8 for x in moff[:-1]) == set(range(8))        # the members start on every alignment
    rc, out, off, st = call(lib, members)
    assert rc == 0, lib.l.ssg_last_error()
    assert (st == 0).all(), np.nonzero(st)[0][:8]
    want = np.zeros(len(payloads) + 1, dtype=np.uint64)
    want[1:] = np.cumsum([len(p) for p in payloads])
    assert (off == want).all()
    whole = out.tobytes()
    bad = [(i, len(p)) for i, p in enumerate(payloads) if whole[int(off[i]):int(off[i + 1])] != p]
    assert not bad, bad[:8]


# ---------------------------------------------------------------- 1. round trip against zlib, every block type

@functools.lru_cache(maxsize=None)
def shaped_payloads():
    rng = np.random.RandomState(7)
    blocks = []
    for k, n in enumerate(BLOCK_LENGTHS):
        blocks += [text_shaped(rng, n), run_shaped(rng, n), rng.bytes(n), bam_shaped(n, k)]
    return blocks


@functools.lru_cache(maxsize=None)
def zlib_members():
    payloads, members = [], []
    for level in (0, 1, 6, 9):
        for k, p in enumerate(shaped_payloads()):
            s = deflate(p, level)
            if level == 0 and p:
                assert s[0] & 6 == 0                                      # stored
            payloads.append(p); members.append(member(s, p, pad=(0, 5, 0, 7)[k % 4] if len(s) < 60000 else 0))
    return members, payloads


@functools.lru_cache(maxsize=None)
def strategy_members():
    rng = np.random.RandomState(19)
    payloads, members = [], []
    some = [f(n) for n in (3, 257, 4097) for f in (lambda n: text_shaped(rng, n), lambda n: run_shaped(rng, n), lambda n: rng.bytes(n), lambda n: bam_shaped(n, 2))] + [bam_shaped(0xff00, 9)]
    for k, p in enumerate(some):
        if k % 4 != 2 or k == 12:                                         # (noise does not shrink: zlib stores it whatever the strategy)
            s = deflate(p, 6, 8, zlib.Z_FIXED)
            assert s[0] & 6 == 2                                          # the fixed code
            payloads.append(p); members.append(member(s, p))
        for strategy in (zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE):
            payloads.append(p); members.append(member(deflate(p, 6, 8, strategy), p))
    # memLevel 1: many dynamic blocks in one member
    p = bam_shaped(0xff00, 4)
    s1, s8 = deflate(p, 6, 1), deflate(p, 6, 8)
    assert len(s1) > len(s8)
    payloads.append(p); members.append(member(s1, p))
    # a flush in the middle: an empty stored block (and, after a sync flush, the re-alignment behind it), several blocks of mixed types
    for flush in (zlib.Z_FULL_FLUSH, zlib.Z_SYNC_FLUSH):
        p = text_shaped(rng, 3001) + bam_shaped(5000, 6)
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        s = c.compress(p[:1234]) + c.flush(flush) + c.compress(p[1234:4000]) + c.flush(flush) + c.compress(p[4000:]) + c.flush()
        assert b"\x00\x00\xff\xff" in s
        payloads.append(p); members.append(member(s, p))
    # a non-final stored block between two Huffman blocks, not on a byte boundary before its LEN
    p = bam_shaped(700, 1) + rng.bytes(900) + text_shaped(rng, 800)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    s = c.compress(p[:700]) + c.flush(zlib.Z_FULL_FLUSH)
    c0 = zlib.compressobj(0, zlib.DEFLATED, -15)
    s += c0.compress(p[700:1600]) + c0.flush(zlib.Z_FULL_FLUSH)
    s += c.compress(p[1600:]) + c.flush()
    payloads.append(p); members.append(member(s, p))
    # bytes behind the final block's end are no error; the end-of-file marker is a good member
    p = b"trailing bytes behind the stream\n" * 9
    payloads.append(p); members.append(member(deflate(p) + b"\x00\xa5\xff", p))
    payloads.append(b""); members.append(EOF_MARKER)
    return members, payloads


def test_emu_inflate_zlib_members(emu_lib):
    check_good(emu_lib, *zlib_members(), every_alignment=True)


@pytest.mark.gpu
def test_gpu_inflate_zlib_members(gpu_lib):
    check_good(gpu_lib, *zlib_members(), every_alignment=True)


def test_emu_inflate_strategies_flushes_and_many_blocks(emu_lib):
    check_good(emu_lib, *strategy_members())


@pytest.mark.gpu
def test_gpu_inflate_strategies_flushes_and_many_blocks(gpu_lib):
    check_good(gpu_lib, *strategy_members())


def check_own_deflate(lib):
    """the device inflates what the device deflated"""
    payloads = shaped_payloads()
    blob = np.frombuffer(b"".join(payloads), dtype=np.uint8)
    cut = np.zeros(len(payloads) + 1, dtype=np.uint64)
    cut[1:] = np.cumsum([len(p) for p in payloads])
    out, off, _ = capi.bgzf_compress(lib, blob, cut)
    whole = out.tobytes()
    members = [whole[int(off[i]):int(off[i + 1])] for i in range(len(payloads))]
    check_good(lib, members, payloads)
    rc, o2, off2, st = capi.bgzf_inflate(lib, out, off)                  # ... and through the Python wrapper
    assert rc == 0 and o2.tobytes() == blob.tobytes() and (off2 == cut).all() and (st == 0).all()


def test_emu_inflate_own_deflate(emu_lib):
    check_own_deflate(emu_lib)


@pytest.mark.gpu
def test_gpu_inflate_own_deflate(gpu_lib):
    check_own_deflate(gpu_lib)


# ---------------------------------------------------------------- 2. hand-made streams

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class Bits:
    """a deflate bit stream: values lowest bit first, Huffman codes highest bit first"""
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255); self.acc >>= 8; self.n -= 8

    def code(self, c, n):
        self.put(int(format(c, "0%db" % n)[::-1], 2), n)

    def block(self, final, btype):
        self.put(final, 1); self.put(btype, 2)

    def sym(self, s):                                                     # the fixed literal/length code
        if s < 144: self.code(0x30 + s, 8)
        elif s < 256: self.code(0x190 + s - 144, 9)
        elif s < 280: self.code(s - 256, 7)
        else: self.code(0xc0 + s - 280, 8)

    def lits(self, data):
        for b in data: self.sym(b)

    def match(self, length, dist):
        i = max(k for k in range(29) if LEN_BASE[k] <= length and (k == 28 or length < 258))
        self.sym(257 + i); self.put(length - LEN_BASE[i], LEN_EXTRA[i])
        j = max(k for k in range(30) if DIST_BASE[k] <= dist)
        self.code(j, 5); self.put(dist - DIST_BASE[j], DIST_EXTRA[j])

    def done(self):
        if self.n: self.out.append(self.acc & 255); self.acc = 0; self.n = 0
        return bytes(self.out)


def fixed_stream(ops):
    """one final block of the fixed code: ops are bytes (literals) or (length, distance)"""
    b = Bits(); b.block(1, 1)
    for op in ops:
        if isinstance(op, bytes): b.lits(op)
        else: b.match(*op)
    b.sym(256)
    return b.done()


@functools.lru_cache(maxsize=None)
def handmade_members():
    rng = np.random.RandomState(23)
    streams = []
    streams.append(fixed_stream([b"a"] + [(258, 1)] * 253 + [(5, 1)]))                      # length 258 at distance 1 up to 0xff00
    for dist in (2, 3, 63, 64, 65):                                                        # the source written in the step just before, dist < len
        for length in (3, 64, 65, 258):
            streams.append(fixed_stream([rng.bytes(dist), (length, dist)]))
    far = rng.bytes(32768)
    streams.append(fixed_stream([far, (3, 32768), b"xyz", (258, 32768 + 6 - 3), (258, 32768)]))   # distance exactly 32768 (and the 13 extra bits just below it)
    streams.append(fixed_stream([b"0123456789", (10, 10)]))                                # a match that ends exactly at ISIZE
    streams.append(fixed_stream([rng.bytes(64), (10, 1), b"!"]))                           # source: the last byte of the previous batch of 64 symbols
    streams.append(fixed_stream([rng.bytes(63), (70, 1), (3, 70), (200, 2), b"q", (258, 1)]))  # matches reading matches of the same batch
    streams.append(fixed_stream([b"ab"] + [(258, 2)] * 253 + [(257, 2), (3, 1)]))                    # a member of 65536 bytes
    payloads = [zlib.decompress(s, -15) for s in streams]
    assert len(payloads[0]) == 0xff00 and len(payloads[-1]) == 65536 and len(payloads[21]) == 32768 + 3 + 3 + 258 + 258
    return [member(s, p) for s, p in zip(streams, payloads)], payloads


def test_emu_inflate_handmade_fixed_streams(emu_lib):
    check_good(emu_lib, *handmade_members())


@pytest.mark.gpu
def test_gpu_inflate_handmade_fixed_streams(gpu_lib):
    check_good(gpu_lib, *handmade_members())


# ---------------------------------------------------------------- 3. malformed members

def canon(lens):
    """canonical codes of a {symbol: length} set (RFC 1951 3.2.2)"""
    code, out = 0, {}
    for n in range(1, 16):
        for s in sorted(k for k, v in lens.items() if v == n):
            out[s] = (code, n); code += 1
        code <<= 1
    return out


def dyn_header(b, hlit, hdist, cl_lens, items, final=1):
    """a dynamic block's header: the code-length code from cl_lens, then items (code-length symbol, value of its extra bits)"""
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    b.block(final, 2); b.put(hlit - 257, 5); b.put(hdist - 1, 5); b.put(19 - 4, 4)
    for s in order: b.put(cl_lens.get(s, 0), 3)
    cc = canon(cl_lens)
    for s, x in items:
        b.code(*cc[s])
        if s >= 16: b.put(x, {16: 2, 17: 3, 18: 7}[s])


FLAT4 = dict((s, 4) for s in range(16))                                   # code-length code: sixteen codes of four bits for the lengths 0..15


@functools.lru_cache(maxsize=None)
def malformed_cases():
    """(name, member, expected status): every one is refused by zlib (asserted in check_malformed)"""
    rng = np.random.RandomState(29)
    p = bam_shaped(5000, 8)
    s = deflate(p)
    assert s[0] & 6 == 4                                                  # a dynamic block
    cases = []
    for cut in (3, 12, len(s) // 3, len(s) // 2, len(s) - 2):             # inside the dynamic header (twice), inside the codes, before the end-of-block
        cases.append(("truncated at %d" % cut, member(s[:cut], p), 1))
    cases.append(("BTYPE 3", frame(b"\x07\x00\x00", 0, 0), 1))
    cases.append(("LEN / NLEN", frame(b"\x01\x05\x00\xfb\xff" + b"hello", zlib.crc32(b"hello"), 5), 1))
    cases.append(("distance beyond the start", frame(fixed_stream([b"a", (3, 2)]), zlib.crc32(b"aaaa"), 4), 1))
    b = Bits(); b.block(1, 1); b.lits(b"abc"); b.sym(257); b.code(30, 5); b.sym(256)
    cases.append(("distance code 30", frame(b.done(), zlib.crc32(b"abcabc"), 6), 1))
    b = Bits(); b.block(1, 1); b.lits(b"abc"); b.sym(286); b.sym(256)
    cases.append(("literal/length 286", frame(b.done(), zlib.crc32(b"abc"), 3), 1))
    b = Bits(); dyn_header(b, 257, 1, {0: 1, 8: 1, 9: 1}, []); b.put(0, 32)
    cases.append(("over-subscribed code-length code", frame(b.done(), 0, 0), 1))
    b = Bits(); dyn_header(b, 257, 1, {0: 2, 8: 2, 9: 2}, []); b.put(0, 32)
    cases.append(("incomplete code-length code", frame(b.done(), 0, 0), 1))
    b = Bits(); dyn_header(b, 257, 1, FLAT4, [(8, 0)] * 257 + [(1, 0)]); b.put(0, 32)
    cases.append(("over-subscribed literal/length code", frame(b.done(), 0, 0), 1))
    b = Bits(); dyn_header(b, 257, 1, FLAT4, [(2, 0) if k in (97, 256) else (0, 0) for k in range(257)] + [(1, 0)]); b.put(0, 32)
    cases.append(("incomplete literal/length code", frame(b.done(), 0, 0), 1))
    b = Bits(); dyn_header(b, 257, 2, FLAT4, [(1, 0) if k in (97, 256) else (0, 0) for k in range(257)] + [(2, 0), (0, 0)]); b.put(0, 32)
    cases.append(("incomplete distance code of more than one bit", frame(b.done(), 0, 0), 1))
    b = Bits(); dyn_header(b, 257, 1, {8: 1, 16: 1}, [(16, 0)]); b.put(0, 32)
    cases.append(("repeat code 16 first", frame(b.done(), 0, 0), 1))
    b = Bits(); dyn_header(b, 257, 1, {8: 1, 18: 1}, [(18, 127), (18, 127)]); b.put(0, 32)
    cases.append(("repeat past HLIT + HDIST", frame(b.done(), 0, 0), 1))
    b = Bits(); dyn_header(b, 257, 1, FLAT4, [(8, 0)] * 256 + [(0, 0), (1, 0)]); b.put(0, 64)
    cases.append(("no end-of-block code", frame(b.done(), 0, 0), 1))
    b = Bits(); dyn_header(b, 288, 1, FLAT4, []); b.put(0, 32)
    cases.append(("HLIT above 286", frame(b.done(), 0, 0), 1))
    cases.append(("ISIZE one too small", frame(s, zlib.crc32(p), len(p) - 1), 2))
    cases.append(("ISIZE one too large", frame(s, zlib.crc32(p), len(p) + 1), 2))
    cases.append(("more blocks behind ISIZE bytes", frame(b"\x00\x64\x00\x9b\xff" + p[:100] + s, zlib.crc32(p[:100]), 100), 2))
    cases.append(("stored block longer than what is left of ISIZE", frame(deflate(p[:300], 0), zlib.crc32(p[:200]), 200), 2))
    cases.append(("a flipped CRC-32 byte", frame(s, zlib.crc32(p) ^ 0x00010000, len(p)), 3))
    return cases


@functools.lru_cache(maxsize=None)
def bit_flips():
    """40 single-bit flips of one level-6 member's stream, each judged by zlib: (member, good by zlib's rule)"""
    rng = np.random.RandomState(31)
    p = bam_shaped(3000, 12)
    s = bytearray(deflate(p))
    out = []
    for pos in sorted(rng.choice(len(s) * 8, 40, replace=False)):
        t = bytearray(s); t[pos >> 3] ^= 1 << (pos & 7)
        m = member(bytes(t), p)
        out.append((m, zlib_verdict(m)[0]))
    return out


MALFORMED_BIN = os.path.join(ROOT, "tests", "golden", "bgzf_inflate_malformed.bin")


def malformed_file_bytes():
    """the malformed members and the bit flips as tools/dbg/inflate_fuzz.cpp reads them: u32 count, then u32 length + bytes each"""
    ms = [m for _, m, _ in malformed_cases()] + [m for m, _ in bit_flips()]
    return struct.pack("<I", len(ms)) + b"".join(struct.pack("<I", len(m)) + m for m in ms)


def test_malformed_set_of_the_fuzz_program_is_current():
    """tests/golden/bgzf_inflate_malformed.bin holds the members of this module (`python tests/test_bgzf_inflate.py` writes it)"""
    assert open(MALFORMED_BIN, "rb").read() == malformed_file_bytes()


def check_malformed(lib):
    rng = np.random.RandomState(37)
    goods = [bam_shaped(2000 + 37 * k, k) for k in range(8)]
    good_m = [member(deflate(g, (1, 6, 9, 0)[k % 4]), g) for k, g in enumerate(goods)]
    cases = malformed_cases()
    for name, m, want in cases:
        assert not zlib_verdict(m)[0], name                              # zlib refuses it: the fixture is what it is meant to be
    flips = bit_flips()
    assert sum(1 for _, ok in flips if not ok) >= 30
    bad = [(name, m, want) for name, m, want in cases] + [("bit flip %d" % k, m, 0 if ok else None) for k, (m, ok) in enumerate(flips)]
    members, expect = [], []
    for k, (name, m, want) in enumerate(bad):                             # a good neighbour on both sides of every bad member
        members += [good_m[k % 8], m]; expect += [(k % 8, 0), (name, want)]
    members.append(good_m[0]); expect.append((0, 0))
    rc, out, off, st = call(lib, members)
    assert rc == SSG_EIO, (rc, lib.l.ssg_last_error())
    assert b"bad member" in lib.l.ssg_last_error()
    isz = [struct.unpack("<I", m[-4:])[0] for m in members]
    assert [int(x) for x in off] == [0] + list(np.cumsum(isz))
    whole = out.tobytes()
    wrong = []
    for i, (what, want) in enumerate(expect):
        got = int(st[i])
        if isinstance(what, int):
            if got != 0 or whole[int(off[i]):int(off[i + 1])] != goods[what]: wrong.append((i, "good neighbour", got))
        elif want is None:
            if got not in (1, 2, 3): wrong.append((i, what, got))
        elif got != want: wrong.append((i, what, got, want))
        elif want == 0 and whole[int(off[i]):int(off[i + 1])] != zlib_verdict(members[i])[1]: wrong.append((i, what, "bytes"))
    assert not wrong, wrong[:10]
    # each bad member alone, and as the only bad one among good ones: the same verdict
    for name, m, want in cases[:8]:
        rc, out, off, st = call(lib, [m])
        assert rc == SSG_EIO and int(st[0]) == want, (name, rc, st)
    # status = NULL: the return code alone
    rc, out, off, st = call(lib, [good_m[1], cases[5][1], good_m[2]], want_status=False)
    assert rc == SSG_EIO and out[:len(goods[1])].tobytes() == goods[1] and out[int(off[2]):].tobytes() == goods[2]


def test_emu_inflate_malformed_members(emu_lib):
    check_malformed(emu_lib)


@pytest.mark.gpu
def test_gpu_inflate_malformed_members(gpu_lib):
    check_malformed(gpu_lib)


# ---------------------------------------------------------------- 4. edges of the entry point

def check_edges(lib):
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    # no member: out_off[0] = 0, nothing else
    off = np.full(1, 77, dtype=np.uint64)
    out = np.full(64, 0xAB, dtype=np.uint8)
    assert lib.l.ssg_bgzf_inflate(None, ptr(np.zeros(1, dtype=np.uint64)), C.c_long(0), ptr(out), C.c_uint64(0), ptr(off), None) == 0
    assert int(off[0]) == 0 and (out == 0xAB).all()
    payloads = [bam_shaped(3000, 1), b"ab", run_shaped(np.random.RandomState(3), 700), b""]
    members = [member(deflate(p), p) for p in payloads]
    # status = NULL
    rc, out, off, _ = call(lib, members, want_status=False)
    assert rc == 0 and out.tobytes() == b"".join(payloads)
    # out_cap one byte short: SSG_EOVERFLOW, nothing behind out + out_cap (call() checks the guard), nothing before it either; the exact size is enough
    need = sum(len(p) for p in payloads)
    rc, out, off, _ = call(lib, members, cap=need - 1)
    assert rc == SSG_EOVERFLOW and (out == 0xAB).all()
    rc, out, off, st = call(lib, members, cap=need)
    assert rc == 0 and out.tobytes() == b"".join(payloads) and (st == 0).all()
    # headers the host refuses, with the member's index in the message
    good = members[0]
    no_bc = bytearray(good); no_bc[12:14] = b"XY"
    bsize = bytearray(good); bsize[16:18] = struct.pack("<H", len(good))
    not_gz = bytearray(good); not_gz[1] = 0x8c
    no_extra = bytearray(good); no_extra[3] = 0
    big = bytearray(good); big[-4:] = struct.pack("<I", 65537)
    for bad, word in ((bytes(no_bc), b"BC"), (bytes(bsize), b"BSIZE"), (bytes(not_gz), b"gzip"), (bytes(no_extra), b"FEXTRA"), (bytes(big), b"ISIZE"), (good[:27], b"28")):
        rc, out, off, _ = call(lib, [members[1], members[2], bad, members[0]], cap=70000)
        msg = lib.l.ssg_last_error()
        assert rc == SSG_EINVAL and b"member 2" in msg and word in msg, (rc, msg)
        assert (out == 0xAB).all()
    # only empty members
    rc, out, off, st = call(lib, [EOF_MARKER] * 5)
    assert rc == 0 and len(out) == 0 and (off == 0).all() and (st == 0).all()
    # the wrapper
    rc, out, off, st = capi.bgzf_inflate(lib, b"".join(members), concat(members)[1])
    assert rc == 0 and out.tobytes() == b"".join(payloads) and (st == 0).all()
    rc, out, off, st = capi.bgzf_inflate(lib, b"".join(members), concat(members)[1], want_status=False)
    assert rc == 0 and st is None and out.tobytes() == b"".join(payloads)


def test_emu_inflate_edges(emu_lib):
    check_edges(emu_lib)


@pytest.mark.gpu
def test_gpu_inflate_edges(gpu_lib):
    check_edges(gpu_lib)


# ---------------------------------------------------------------- 5. across the per-call batch

@functools.lru_cache(maxsize=None)
def batch_members():
    """4097 members: 4096 of three bytes and, behind them, one of the largest size -- the second device call's"""
    rng = np.random.RandomState(13)
    payloads = [rng.bytes(3) for _ in range(4096)] + [bam_shaped(0xff00, 5)]
    return [member(deflate(p), p) for p in payloads], payloads


def test_emu_inflate_across_the_per_call_batch(emu_lib):
    check_good(emu_lib, *batch_members())


@pytest.mark.gpu
def test_gpu_inflate_across_the_per_call_batch(gpu_lib):
    check_good(gpu_lib, *batch_members())


# ---------------------------------------------------------------- 6. the readers

LOG_RE = re.compile(r"\[sambamba\] inflate: (\d+) members on the device, (\d+) stored members copied, (\d+) on the host")


def run_reader(sambamba, args, device, **kw):
    env = dict(os.environ)
    for k in ("SSG_BGZF_INFLATE_DEVICE", "SSG_BGZF_INFLATE_LOG"): env.pop(k, None)
    if device: env.update(SSG_BGZF_INFLATE_DEVICE="1", SSG_BGZF_INFLATE_LOG="1")
    return subprocess.run([sambamba] + args, capture_output=True, env=env, **kw)


def check_readers(sambamba, tmp_path):
    d = str(tmp_path)
    write_sam(d + "/in.sam")
    lines = open(d + "/in.sam").read().split("\n")
    hdr = [l for l in lines if l.startswith("@")]
    body = [l for l in lines if l and not l.startswith("@")]
    for name, part in (("a", body[:len(body) // 2]), ("b", body[len(body) // 2:]), ("s", body)):
        with open("%s/%s.sam" % (d, name), "w") as f: f.write("\n".join(hdr + part) + "\n")
        with open("%s/%s.sam" % (d, name), "rb") as fi, open("%s/%s.u.bam" % (d, name), "wb") as fo:
            subprocess.run([sambamba, "view", "-S", "-f", "bam", "-l", "0", "/dev/stdin"], stdin=fi, stdout=fo, check=True)
        subprocess.run([sambamba, "sort", "-t", "4", "-m", "1G", "--tmpdir=%s/tmp_%s" % (d, name), "-o", "%s/%s.bam" % (d, name), "%s/%s.u.bam" % (d, name)], check=True, capture_output=True)
        os.unlink("%s/%s.bam.bai.ssg" % (d, name))                       # `index` computes from the file
    subprocess.run([sambamba, "sort", "-t", "4", "-l", "0", "-m", "1G", "--tmpdir=%s/tmp_s0" % d, "-o", d + "/s0.bam", d + "/s.u.bam"], check=True, capture_output=True)
    os.unlink(d + "/s0.bam.bai.ssg")
    got = {}
    for device in (False, True):
        tag = "dev" if device else "host"
        logs = []
        os.path.exists(d + "/s.bam.bai") and os.unlink(d + "/s.bam.bai")
        r = run_reader(sambamba, ["index", "-t", "4", d + "/s.bam"], device); assert r.returncode == 0, r.stderr[-800:]
        logs.append(r.stderr.decode()); bai = open(d + "/s.bam.bai", "rb").read()
        r = run_reader(sambamba, ["flagstat", "-t", "4", d + "/s.bam"], device); assert r.returncode == 0, r.stderr[-800:]
        logs.append(r.stderr.decode()); flag = r.stdout
        r = run_reader(sambamba, ["merge", "-t", "4", "%s/m_%s.bam" % (d, tag), d + "/a.bam", d + "/b.bam"], device); assert r.returncode == 0, r.stderr[-800:]
        logs.append(r.stderr.decode()); merged = open("%s/m_%s.bam" % (d, tag), "rb").read()
        r = run_reader(sambamba, ["view", "-h", d + "/s.bam"], device); assert r.returncode == 0, r.stderr[-800:]
        logs.append(r.stderr.decode()); sam = r.stdout
        # the stored stream of `view -l 0` / `sort -l 0`: copied on the host, nothing on the device
        os.path.exists(d + "/s0.bam.bai") and os.unlink(d + "/s0.bam.bai")
        r = run_reader(sambamba, ["index", "-t", "4", d + "/s0.bam"], device); assert r.returncode == 0, r.stderr[-800:]
        stored_log = r.stderr.decode(); bai0 = open(d + "/s0.bam.bai", "rb").read()
        got[tag] = (bai, flag, merged, sam, bai0)
        if device:
            for k, log in enumerate(logs):
                ms = LOG_RE.findall(log)
                assert len(ms) == (2 if k == 2 else 1), (k, log[-800:])   # one line per reader: merge has two
                for m in ms: assert int(m[0]) > 0 and int(m[2]) == 0, (k, log[-800:])
            ms = LOG_RE.findall(stored_log)
            assert len(ms) == 1 and int(ms[0][0]) == 0 and int(ms[0][1]) > 0, stored_log[-800:]
        else:
            assert not any(LOG_RE.search(l) for l in logs + [stored_log])
    assert got["dev"][0] == got["host"][0] and len(got["host"][0]) > 100   # the .bai
    assert got["dev"][1] == got["host"][1] and b"6000 + 0 in total" in got["host"][1]
    assert got["dev"][2] == got["host"][2] and len(got["host"][2]) > 100000
    assert got["dev"][3] == got["host"][3] and got["host"][3].count(b"\n") == 6000 + len(hdr)
    assert got["dev"][4] == got["host"][4]
    # one corrupted member: `index` exits 1 with the member's offset, under both settings
    bam = bytearray(open(d + "/s.bam", "rb").read())
    o, starts = 0, []
    while o < len(bam): starts.append(o); o += struct.unpack_from("<H", bam, o + 16)[0] + 1
    assert len(starts) > 6
    victim = starts[3]
    bam[victim + 18 + 40] ^= 0x10
    bam[victim + 18 + 41] ^= 0xff
    m = bytes(bam[victim:starts[4]])
    assert not zlib_verdict(m)[0]
    try:
        zlib.decompressobj(-15).decompress(m[18:-8])
        refused = False
    except zlib.error:
        refused = True
    assert refused                                                       # (the host path checks the stream only: the damage must show there)
    open(d + "/bad.bam", "wb").write(bytes(bam))
    for device in (False, True):
        r = run_reader(sambamba, ["index", "-t", "4", d + "/bad.bam"], device)
        assert r.returncode == 1 and b"inflate failed" in r.stderr and (b"offset %d" % victim) in r.stderr, r.stderr[-800:]


def test_emu_sambamba_readers_with_device_inflate(tmp_path, emu_lib):
    check_readers(os.path.join(ROOT, "tests", "emu", "sambamba_emu"), tmp_path)


@pytest.mark.gpu
def test_gpu_sambamba_readers_with_device_inflate(tmp_path, gpu_lib):
    check_readers(os.path.join(ROOT, "bin", "sambamba"), tmp_path)


if __name__ == "__main__":
    open(MALFORMED_BIN, "wb").write(malformed_file_bytes())
