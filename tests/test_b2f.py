"""bamtofastq on the device (k_b2f.h; ssg_b2f_create / push / waiting): eligibility, pairing, order and the FASTQ text decided and written on the device, against
tests/b2f_reference.py -- a plain-Python model that shares no code with the kernels or with bamkit -- and `bamkit bamtofastq' with SSG_B2F_DEVICE=1 against the
same command without it and against the model.  Every edge of the text kernel (lengths around a wave's dwords, every output alignment, both orientations, all
16 codes), of the aux walk, of the state machine across names, hashes and pushes, every refusal.  CPU-side on the host emulation of the kernels; `-m gpu' on the
MI355X."""
import ctypes as C
import functools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import b2f_reference as ref
from common import ROOT
from speedseq_amd import capi
from test_bam_scan import CTG, OURS, concat, make_member, payload_of, reblock, rec, small_members

SSG_EIO, SSG_EINVAL, SSG_ERANGE, SSG_EALIGN, SSG_EOVERFLOW = -5, -22, -34, -71, -75
P, R, F, L = 0x1, 0x10, 0x40, 0x80


def mk(name, flag, codes=(), quals=None, aux=b"", cigar=(), l_qname_0=False):
    """a record of rec() with these bases (4-bit codes) and qualities"""
    l = len(codes)
    r = bytearray(rec(0, 100, flag, cigar, name=b"" if l_qname_0 else name + b"\0", l_seq=l, extra=aux))
    o = 36 + (0 if l_qname_0 else len(name) + 1) + 4 * len(cigar)
    for i, c in enumerate(codes):
        r[o + (i >> 1)] |= c << (0 if i & 1 else 4)
    if quals is not None:
        r[o + (l + 1) // 2:o + (l + 1) // 2 + l] = bytes(quals)
    return bytes(r)


def codes_of(n, k=0):
    return [(i + k) % 16 for i in range(n)]


def quals_of(n, k=0):
    return [(i * 7 + k) % 94 for i in range(n)]


def pair(name, l1=5, l2=5, f1=P | F, f2=P | L, aux1=b"", aux2=b"", k=0):
    return [mk(name, f1, codes_of(l1, k), quals_of(l1, k), aux1), mk(name, f2, codes_of(l2, k + 3), quals_of(l2, k + 5), aux2)]


def group(recs, sizes=(3, 1, 2)):
    """the records as members' payloads of 3, 1, 2, 3, ... records: every member begins at a record"""
    out, i, k = [], 0, 0
    while i < len(recs):
        out.append(b"".join(recs[i:i + sizes[k % len(sizes)]]))
        i += sizes[k % len(sizes)]
        k += 1
    return out


class Stream:
    """one store and one ssg_b2f_t with the model next to them"""

    def __init__(self, lib, rg=(), rename=False, hash_bits=64, cap=1 << 40):
        self.lib, self.rg, self.rename = lib, rg, rename
        self.recs = capi.recs_create(lib, cap)
        self.b = capi.b2f_create(lib, self.recs, rg, rename, hash_bits)
        self.model = ref.Model(rg, rename)

    def append(self, records):
        payloads = group(records)
        blob, moff = concat([make_member(p, ("stored", "fixed", "dynamic")[k % 3]) for k, p in enumerate(payloads)])
        rc, cid, off, st = capi.recs_append_bgzf(self.lib, self.recs, blob, moff)
        assert rc == 0 and (st == 0).all(), self.lib.l.ssg_last_error()
        return cid, off

    def push(self, records, **kw):
        """one push, held to the model: returns the text"""
        cid, off = self.append(records)
        carried = capi.b2f_waiting(self.lib, self.b)[1]
        rc, text, n, n_rec, n_pairs = capi.b2f_push(self.lib, self.b, cid, off, **kw)
        assert rc == 0, self.lib.l.ssg_last_error()
        want, w_rec, w_pairs = self.model.push(b"".join(records))
        assert (n_rec, n_pairs) == (w_rec, w_pairs)
        assert text == want, first_difference(text, want)
        assert len(text) <= 2 * (int(off[-1]) + carried) + 64            # the documented bound
        assert capi.b2f_waiting(self.lib, self.b) == self.model.held()
        with pytest.raises(capi.SsgError):                                # the chunk is released
            capi.recs_release(self.lib, self.recs, cid)
        return text

    def close(self):
        self.b.close()
        self.recs.close()


def first_difference(a, b):
    k = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
    return "lengths %d / %d, first difference at %d: %r / %r" % (len(a), len(b), k, a[max(0, k - 30):k + 30], b[max(0, k - 30):k + 30])


def heads(text):
    """the first line of every half"""
    return text.split(b"\n")[0:-1:4]


def once(lib, records, **kw):
    s = Stream(lib, **kw)
    text = s.push(records)
    s.close()
    return text


# ---- the text ----
def check_text_lengths(lib):
    recs = []
    for k, l in enumerate((0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 310)):
        recs += pair(b"len%d" % l, l, l, P | F | (R if k % 2 else 0), P | L | (0 if k % 2 else R), k=k)
    recs += pair(b"sixteen_f", 16, 16) + pair(b"sixteen_r", 16, 16, P | F | R, P | L | R)            # all 16 codes, both orientations
    recs += [mk(b"q", P | F, codes_of(94), list(range(94))), mk(b"q", P | L | R, codes_of(94), list(range(94)))]
    recs += [mk(b"noq", P | F, codes_of(7), [0xff] + [3] * 6), mk(b"noq", P | L | R, codes_of(7), [0xff] * 7), mk(b"ff2", P | F, codes_of(3), [1, 0xff, 2]), mk(b"ff2", P | L, codes_of(3), [0xde, 0xff, 0])]
    text = once(lib, recs)
    assert text.count(b"\n") == 4 * len(recs) and b"@len0/1\n\n+\n\n" in text and b"IIIIIII\n" in text


def check_names(lib):
    recs = []
    for nl in (0, 1, 2, 3, 4, 5, 254):
        recs += pair(b"n" * nl, 4 + nl % 3, 9, k=nl)
    once(lib, recs)
    # l_qname == 0: an empty name too, in a stream of its own
    text = once(lib, [mk(b"", P | F, codes_of(5), quals_of(5), l_qname_0=True), mk(b"x", P | F, codes_of(2)), mk(b"", P | L, codes_of(6), quals_of(6), l_qname_0=True)])
    assert text.startswith(b"@/1\n")


RG_AUX = {
    "absent": b"NMC\x01",
    "present": b"NMC\x01RGZgrp1\0",
    "twice": b"RGZone\0XSi\1\0\0\0RGZtwo\0",
    "behind_B": b"XBBs\3\0\0\0" + bytes(6) + b"RGZarr\0",
    "behind_d": b"XDd" + bytes(8) + b"RGZhidden\0",
    "Z_swallows_it": b"XZZopen" + b"RGZgone\0",
    "unterminated_Z_behind_it": b"RGZkept\0XZZno end",
    "truncated_B": b"RGZkeptB\0XBBi\1",
    "H_is_not_Z": b"RGH1f\0",
    "empty": b"RGZ\0",
    "fixed_types": b"aaAxbbc\1ccC\1dds\1\0eeS\1\0ffi\1\0\0\0ggI\1\0\0\0hhf\0\0\0\0RGZafter\0",
}


def check_read_groups(lib):
    recs = []
    for k, (name, aux) in enumerate(RG_AUX.items()):
        recs += pair(name.encode(), 6, 7, aux1=aux, aux2=RG_AUX["present"] if k % 2 else aux, k=k)   # (every second pair: halves with different RGs)
    text = once(lib, recs)
    for name, rg in (("absent", None), ("present", b"grp1"), ("twice", b"two"), ("behind_B", b"arr"), ("behind_d", None), ("Z_swallows_it", None), ("unterminated_Z_behind_it", b"kept"),
                     ("truncated_B", b"keptB"), ("H_is_not_Z", None), ("empty", None), ("fixed_types", b"after")):
        assert (b"@%s/1" % name.encode() + (b" RG:Z:" + rg if rg else b"") + b"\n") in text, name


def check_alignments(lib):
    for nl in range(1, 9):                                                  # the second pair's text begins at every offset mod 4, and so does every half behind it
        once(lib, pair(b"a" * nl, 3, 3) + pair(b"second", 70, 33, P | F | R, P | L, aux1=RG_AUX["present"]) + pair(b"third", 1, 2))


# ---- who takes part ----
def check_eligibility(lib):
    H = (4, 5)
    recs = [mk(b"sec", P | F | 0x100, codes_of(4))] + pair(b"sec") + [mk(b"sup", P | L | 0x800, codes_of(4))] + pair(b"sup")
    recs += [mk(b"single", F, codes_of(4)), mk(b"single", L, codes_of(4))]                                                          # not paired
    recs += [mk(b"h_first", P | F, codes_of(4), cigar=[H, (4, 0)]), mk(b"h_first", P | L, codes_of(4)), mk(b"h_first", P | F, codes_of(4), quals_of(4, 9), cigar=[(4, 0)])]
    recs += [mk(b"h_last", P | F, codes_of(4)), mk(b"h_last", P | L, codes_of(4), cigar=[(4, 0), H]), mk(b"h_last", P | L, codes_of(4), quals_of(4, 9))]
    recs += [mk(b"h_mid", P | F, codes_of(4)), mk(b"h_mid", P | L, codes_of(4), cigar=[(2, 0), H, (2, 0)]), mk(b"h_mid", P | L, codes_of(5))]
    text = once(lib, recs)
    assert heads(text) == [b"@sec/1", b"@sec/2", b"@sup/1", b"@sup/2", b"@h_first/1", b"@h_first/2", b"@h_last/1", b"@h_last/2", b"@h_mid/1", b"@h_mid/2"]
    aux = lambda g: b"RGZ" + g + b"\0"
    recs = pair(b"a", aux1=aux(b"lib1"), aux2=aux(b"lib1")) + pair(b"b", aux1=aux(b"lib"), aux2=aux(b"lib")) + pair(b"c", aux1=aux(b"lib1x"), aux2=aux(b"lib1x")) + pair(b"d", aux1=aux(b"lib2"), aux2=aux(b"lib2")) + \
        pair(b"e") + pair(b"f", aux1=aux(b"lib1"), aux2=aux(b"lib2")) + pair(b"g", aux1=aux(b"lib1")) + [mk(b"g", P | L, codes_of(3), aux=aux(b"lib1"))]
    assert len(heads(once(lib, recs, rg=["lib1"]))) == 4                                                                            # a and g; a prefix or an extension of an id is no match
    assert len(heads(once(lib, recs, rg=["lib1", "lib2"]))) == 8 and len(heads(once(lib, recs, rg=["lib2", "nothing"]))) == 2
    assert len(heads(once(lib, recs))) == 14


# ---- the state machine ----
SEQUENCES = [(1, 0), (0, 1), (1, 1, 0), (1, 0, 1), (1, 1, 0, 0), (0, 0), (1, 0, 1, 0)]


def named(name, firsts, k=0):
    return [mk(name, P | (F if f else L), codes_of(3 + i, k), quals_of(3 + i, k)) for i, f in enumerate(firsts)]


def interleave(order, seqs):
    """records of the names in `order' (one letter a record), each name's records in its own sequence"""
    its = {n: iter(named(n.encode(), s, ord(n))) for n, s in seqs.items()}
    return [next(its[n]) for n in order]


def check_state_machine(lib):
    for s in SEQUENCES:
        once(lib, named(b"one", s))
    once(lib, [r for k, s in enumerate(SEQUENCES) for r in named(b"name%d" % k, s, k)])
    two = {"A": (1, 0), "B": (0, 1)}
    for order in ("ABBA", "ABAB", "AABB", "BAAB"):                           # nested, crossing, one completing record directly behind another
        once(lib, interleave(order, two))
    three = {"A": (1, 0, 1, 0), "B": (1, 1, 0), "C": (0, 1)}
    for order in ("ABCABCABA", "AAAABBBCC", "CBACBABAA", "ABACABABC"):
        once(lib, interleave(order, three))


# ---- the hash groups, it does not decide ----
@functools.lru_cache(maxsize=None)
def many_names():
    rng = np.random.RandomState(5)
    recs = []
    for i in range(300):                                                     # 110 whole pairs, the rest single ends and same-end repeats: 410 eligible records
        name = b"read_%d" % i
        recs += [named(name, (1, 0), i), named(name, (0,), i), named(name, (1,), i), named(name, (1, 1), i) if i % 9 == 0 else named(name, (0,), i)][0 if i < 110 else 1 + i % 3]
    order = rng.permutation(len(recs))
    return [recs[i] for i in order]


def check_hash_independence(lib):
    recs = many_names()
    want = once(lib, recs)
    assert len(heads(want)) == 220
    for bits in (8, 2, 1):
        assert once(lib, recs, hash_bits=bits) == want
    two_hundred = [r for i in range(100) for r in named(b"z%d" % i, (1, 0), i)]
    assert once(lib, two_hundred, hash_bits=0) == once(lib, two_hundred)
    # 257 eligible records in one run: refused, nothing changed, and the same chunk goes through another object
    s = Stream(lib, hash_bits=0)
    recs = two_hundred + named(b"tail", (1,) * 57)
    cid, off = s.append(recs)
    rc, text, n, n_rec, n_pairs = capi.b2f_push(lib, s.b, cid, off)
    assert rc == SSG_ERANGE and b"share one name hash" in lib.l.ssg_last_error() and capi.b2f_waiting(lib, s.b) == (0, 0)
    wide = capi.b2f_create(lib, s.recs)
    rc, text, n, n_rec, n_pairs = capi.b2f_push(lib, wide, cid, off)
    assert rc == 0 and text == ref.Model().push(b"".join(recs))[0] and n_pairs == 100 and capi.b2f_waiting(lib, wide)[0] == 1
    wide.close()
    s.close()


# ---- the carry ----
@functools.lru_cache(maxsize=None)
def carry_stream():
    recs = interleave("ABCDEFGHIABCDEFGHICDEGEG", {"A": (1, 0), "B": (0, 1), "C": (1, 1, 0), "D": (1, 0, 1), "E": (1, 1, 0, 0), "F": (0, 0), "G": (1, 0, 1, 0), "H": (0, 1), "I": (1, 0)})
    assert len(recs) == 24
    return recs


def check_carry(lib, cuts_list):
    recs = carry_stream()
    whole = once(lib, recs)
    assert len(heads(whole)) == 2 * 9
    for cuts in cuts_list:
        s = Stream(lib)
        edges = [0] + list(cuts) + [len(recs)]
        parts = [s.push(recs[a:b]) for a, b in zip(edges[:-1], edges[1:])]
        assert b"".join(parts) == whole, cuts
        s.close()


def check_carry_two(lib):
    check_carry(lib, [(c,) for c in range(1, 24)])
    # one end held in chunk 1, the same end and then the other end in chunk 2
    s = Stream(lib)
    assert s.push(named(b"x", (1,)) + named(b"y", (0,))) == b""
    assert s.push(named(b"x", (1, 0), 4)).startswith(b"@x/1\n=AC\n")       # the held one's bases, not the repeat's
    assert capi.b2f_waiting(lib, s.b)[0] == 1
    s.close()


def check_carry_three(lib):
    rng = np.random.RandomState(11)
    check_carry(lib, [tuple(sorted(rng.choice(np.arange(1, 24), size=2, replace=False))) for _ in range(20)])


# ---- -n ----
def check_rename(lib):
    recs = [r for i in range(120) for r in named(b"p%d" % i, (1, 0) if i % 2 else (0, 1), i)] + named(b"lonely", (1,))
    whole = once(lib, recs, rename=True)
    assert whole.startswith(b"@0/1\n") and b"@9/2\n" in whole and b"@10/1\n" in whole and b"@99/2\n" in whole and b"@100/1\n" in whole and b"@119/2\n" in whole and b"@120/" not in whole
    s = Stream(lib, rename=True)
    parts = [s.push(recs[:19]), s.push(recs[19:199]), s.push(recs[199:])]   # the widths change inside the second push; a pair straddles each cut
    assert b"".join(parts) == whole
    s.close()


# ---- room ----
def check_capacity(lib):
    recs = carry_stream()
    want = once(lib, recs)
    s = Stream(lib)
    cid, off = s.append(recs)
    rc, text, n, n_rec, n_pairs = capi.b2f_push(lib, s.b, cid, off, out_cap=len(want) - 1)
    assert rc == SSG_EOVERFLOW and n == len(want) and capi.b2f_waiting(lib, s.b) == (0, 0)
    rc, n_scan, _, _, _ = capi.recs_scan(lib, s.recs, cid, off, 0)                                   # the chunk is still in the store
    assert rc == 0 and n_scan == 24
    rc, text, n, n_rec, n_pairs = capi.b2f_push(lib, s.b, cid, off, out_cap=len(want))
    assert rc == 0 and text == want and n_pairs == 9
    s.close()


# ---- bad streams and refusals ----
def check_refusals(lib):
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    recs = capi.recs_create(lib, 1 << 30)
    for kw, words in ((dict(rg=[None]), b"NULL or empty"), (dict(rg=["a", ""]), b"NULL or empty"), (dict(hash_bits=-1), b"hash_bits"), (dict(hash_bits=65), b"hash_bits")):
        rc, b = capi.b2f_create(lib, recs, raw=True, **kw)
        assert rc == SSG_EINVAL and b is None and lib.l.ssg_last_error().startswith(b"ssg_b2f_create") and words in lib.l.ssg_last_error(), lib.l.ssg_last_error()
    h = C.c_void_p()
    assert lib.l.ssg_b2f_create(None, None, C.c_int(0), C.c_int(0), C.c_int(64), C.byref(h)) == SSG_EINVAL and b"no record store" in lib.l.ssg_last_error()
    assert lib.l.ssg_b2f_create(recs.h, None, C.c_int(-1), C.c_int(0), C.c_int(64), C.byref(h)) == SSG_EINVAL and b"n_rg" in lib.l.ssg_last_error()
    recs.close()

    s = Stream(lib)
    s.push(named(b"held", (1,)))                                             # a state that must survive everything below
    before = capi.b2f_waiting(lib, s.b)
    good = carry_stream()

    def refused(records, want_rc, words, hint=None, first=0, cuts=None, keep=False):
        if cuts is None:
            cid, off = s.append(records)
        else:                                                               # members cut where the caller says
            stream = b"".join(records)
            blob, moff = concat([make_member(stream[a:b], "dynamic") for a, b in zip(cuts[:-1], cuts[1:])])
            rc, cid, off, st = capi.recs_append_bgzf(lib, s.recs, blob, moff)
            assert rc == 0
        rc, text, n, n_rec, n_pairs = capi.b2f_push(lib, s.b, cid, off if hint is None else hint, first=first)
        msg = lib.l.ssg_last_error()
        assert rc == want_rc and msg.startswith(b"ssg_b2f_push: ") and re.search(words, msg), (rc, msg)
        assert text == b"" and n_pairs == 0 and capi.b2f_waiting(lib, s.b) == before
        rc, n_scan, _, _, _ = capi.recs_scan(lib, s.recs, cid, [0, int(off[-1])], 0)                 # the chunk is still there
        assert rc in (0, SSG_EIO)
        if not keep:
            capi.recs_release(lib, s.recs, cid)
        return cid, off

    stream = b"".join(good)
    sizes = [len(r) for r in good]
    at = sum(sizes[:7])
    # the scan's own cases, in the scan's words
    bad = bytearray(stream); struct.pack_into("<I", bad, at, 31)
    refused([bytes(bad)], SSG_EIO, rb"malformed record at offset %d: a block_size below 32" % at, cuts=[0, at, len(stream)])
    bad = bytearray(stream); struct.pack_into("<I", bad, at, 0xffffffff)
    refused([bytes(bad)], SSG_EIO, rb"malformed record at offset %d: it runs past the end" % at, cuts=[0, at, len(stream)])
    bs, = struct.unpack_from("<I", stream, at)
    bad = bytearray(stream); struct.pack_into("<H", bad, at + 16, bs // 4 + 1)
    refused([bytes(bad)], SSG_EIO, rb"malformed record at offset %d: l_qname \+ 4 n_cigar" % at, cuts=[0, at, len(stream)])
    refused([stream], SSG_EALIGN, rb"not record-aligned at hint 0\b", cuts=[0, at - 11, len(stream)])
    # a sequence that overruns its record by one byte: l_seq one more than the record holds, with nothing behind the qualities
    bad = bytearray(mk(b"over", P | F, codes_of(8), quals_of(8), aux=b"\0")); struct.pack_into("<i", bad, 4 + 16, 9)              # (9 + 1) / 2 + 9 = 14 bytes where 4 + 8 + 1 = 13 lie
    refused(good[:5] + [bytes(bad)] + good[5:], SSG_EIO, rb"malformed record at offset %d: 32 \+ l_qname" % sum(sizes[:5]))
    ok = bytearray(mk(b"fits", P | F, codes_of(8), quals_of(8), aux=b"\0\0")); struct.pack_into("<i", ok, 4 + 16, 9)             # one byte more in the record: it ends with its qualities, taken
    # the entry's own refusals
    cid, off = refused(good, SSG_EINVAL, rb"hint\[\] decreases at 0", hint=[5, 0, sum(sizes)], keep=True)
    n_rec, n_pairs, out_len = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    buf = np.zeros(64, dtype=np.uint8)
    hint = np.ascontiguousarray(off, dtype=np.uint64)
    head = (C.c_uint32(cid), ptr(hint), C.c_int64(len(hint) - 1), C.c_uint64(0))
    assert lib.l.ssg_b2f_push(None, *head, ptr(buf), C.c_uint64(64), C.byref(out_len), C.byref(n_rec), C.byref(n_pairs)) == SSG_EINVAL
    assert lib.l.ssg_b2f_push(s.b.h, *head, None, C.c_uint64(64), C.byref(out_len), C.byref(n_rec), C.byref(n_pairs)) == SSG_EINVAL and b"no out" in lib.l.ssg_last_error()
    assert lib.l.ssg_b2f_push(s.b.h, *head, ptr(buf), C.c_uint64(64), None, C.byref(n_rec), C.byref(n_pairs)) == SSG_EINVAL
    assert lib.l.ssg_b2f_push(s.b.h, C.c_uint32(cid + 7), ptr(hint), C.c_int64(len(hint) - 1), C.c_uint64(0), ptr(buf), C.c_uint64(64), C.byref(out_len), C.byref(n_rec), C.byref(n_pairs)) == SSG_EINVAL
    assert b"ssg_b2f_push: chunk %d does not exist" % (cid + 7) in lib.l.ssg_last_error()
    capi.recs_order(lib, s.recs, np.array([cid << 40], dtype=np.uint64), np.array([0, sizes[0]], dtype=np.uint64))
    rc, text, n, _, _ = capi.b2f_push(lib, s.b, cid, off)
    assert rc == SSG_EINVAL and b"an order is declared" in lib.l.ssg_last_error()
    capi.recs_reopen(lib, s.recs)
    assert capi.b2f_waiting(lib, s.b) == before
    # ... and after all of that the object goes on as if nothing had been asked of it
    rc, text, n, n_rec, n_pairs = capi.b2f_push(lib, s.b, cid, off)
    s.model.push(b"")
    assert rc == 0 and text == s.model.push(stream)[0] and capi.b2f_waiting(lib, s.b) == s.model.held()
    s.push([bytes(ok)] + named(b"fits", (0,)) + named(b"held", (0,)))
    s.close()


def check_capacity_of_the_store(lib):
    """the carry counts against the store's capacity: a store sized for one chunk takes the next chunk only when the carry leaves room"""
    held = named(b"h1", (1,)) + named(b"h2", (1,))
    size = sum(len(r) for r in held)
    s = Stream(lib, cap=size)
    s.push(held)
    assert capi.b2f_waiting(lib, s.b) == (2, size)
    one = np.zeros(1, dtype=np.uint8)
    assert lib.l.ssg_recs_append(s.recs.h, one.ctypes.data_as(C.c_void_p), C.c_uint64(1), None) == -12                               # full: the carry is all of it
    s.b.close()
    cid = capi.recs_append(lib, s.recs, one)                                                                                        # freed with the object
    s.recs.close()


CHECKS = {
    "text_lengths": check_text_lengths, "names": check_names, "read_groups": check_read_groups, "alignments": check_alignments, "eligibility": check_eligibility,
    "state_machine": check_state_machine, "hash_independence": check_hash_independence, "carry_two_chunks": check_carry_two, "carry_three_chunks": check_carry_three,
    "rename": check_rename, "capacity": check_capacity, "refusals": check_refusals, "store_capacity": check_capacity_of_the_store,
}


@pytest.mark.parametrize("name", sorted(CHECKS))
def test_emu_b2f(emu_lib, name):
    CHECKS[name](emu_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CHECKS))
def test_gpu_b2f(gpu_lib, name):
    CHECKS[name](gpu_lib)


def test_the_model_on_a_stream_read_by_eye():
    recs = [mk(b"r1", P | F, [1, 2, 4, 8], [0, 1, 2, 3], b"RGZg\0"), mk(b"r2", P | L, [1]), mk(b"r1", P | L | R, [1, 2, 4, 8, 15], [0, 1, 2, 3, 4])]
    text, n, pairs = ref.Model().push(b"".join(recs))
    assert text == b"@r1/1 RG:Z:g\nACGT\n+\n!\"#$\n@r1/2\nNACGT\n+\n%$#\"!\n" and (n, pairs) == (3, 1)
    assert ref.Model(rename=True).push(b"".join(recs))[0].startswith(b"@0/1 RG:Z:g\n")
    assert ref.Model(rg=["other"]).push(b"".join(recs))[0] == b""


# ---------------- bamkit bamtofastq ----------------
def write_pairs_sam(path, seed, n, rgs):
    """n simulated pairs at random places with secondary and supplementary records, some mates missing, two read groups; unsorted"""
    rng = np.random.RandomState(seed)
    lines = []
    for i in range(n):
        ctg, ln = CTG[rng.randint(3)]
        p1 = int(rng.randint(1, ln - 1000)); p2 = p1 + int(rng.randint(50, 600))
        rg = rgs[i % len(rgs)]
        rev1 = int(rng.randint(2))
        for which, pos, rev in ((0, p1, rev1), (1, p2, 1 - rev1)):
            if i % 37 == 5 and which == i % 2:
                continue                                                    # a mate that is not in the file
            l = 100 if i % 11 else 73
            seq = "".join("ACGTN"[b] for b in rng.choice(5, size=l, p=[.24, .24, .24, .24, .04])); qual = "".join(chr(33 + q) for q in rng.randint(2, 41, size=l))
            flag = 1 | (0x40 if which == 0 else 0x80) | (0x10 if rev else 0) | (0x20 if not rev else 0)
            tags = "\tRG:Z:%s\tNM:i:%d" % (rg, i % 4) if i % 50 else "\tNM:i:0"
            lines.append((ctg, pos, "%s_p%d\t%d\t%s\t%d\t60\t%s\t=\t%d\t0\t%s\t%s%s\n" % (rgs[0], i, flag, ctg, pos, "%dM" % l if i % 7 else "10S%dM" % (l - 10), p1 if which else p2, seq, qual, tags)))
            if i % 13 == 3:                                                 # a secondary or a supplementary record of the same read, hard-clipped like bwa's
                lines.append((ctg, pos + 7, "%s_p%d\t%d\t%s\t%d\t0\t30H%dM\t=\t%d\t0\t%s\t%s%s\n" % (rgs[0], i, flag | (0x100 if i % 2 else 0x800), ctg, pos + 7, l - 30, p1, seq[30:], qual[30:], tags)))
    with open(path, "w") as f:
        f.write("@HD\tVN:1.3\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CTG) + "".join("@RG\tID:%s\tSM:s\n" % g for g in rgs))
        f.writelines(l[2] for l in lines)


class Kit:
    """the inputs of a session, made through the product's own view and sort, and runs of bamtofastq on them"""

    def __init__(self, bamkit, sambamba, d):
        self.bamkit, self.d = bamkit, str(d)
        self.clean = {k: v for k, v in os.environ.items() if k not in OURS and not k.startswith("SSG_B2F")}
        for name, seed, n, rgs in (("a", 21, 2000, ("ga", "gb")), ("b", 22, 600, ("gc", "ga"))):
            write_pairs_sam("%s/%s.sam" % (self.d, name), seed, n, rgs)
            with open("%s/%s.sam" % (self.d, name), "rb") as fi, open("%s/%s.u.bam" % (self.d, name), "wb") as fo:
                subprocess.run([sambamba, "view", "-S", "-f", "bam", "/dev/stdin"], stdin=fi, stdout=fo, check=True, env=self.clean)
            subprocess.run([sambamba, "sort", "-t", "4", "-m", "1G", "--tmpdir=%s/tmp_%s" % (self.d, name), "-o", self.path(name), "%s/%s.u.bam" % (self.d, name)], check=True, capture_output=True, env=self.clean)
        open(self.path("skew"), "wb").write(reblock(open(self.path("a"), "rb").read(), step=30011))

    def path(self, name):
        return "%s/%s.bam" % (self.d, name)

    def plain(self, name):
        return payload_of(open(self.path(name), "rb").read())

    def run(self, args, extra, stdin=None):
        env = dict(self.clean, SSG_DEBUG="1"); env.update(extra)
        r = subprocess.run([self.bamkit, "bamtofastq"] + list(args), capture_output=True, env=env, stdin=stdin)
        return r.returncode, r.stdout, r.stderr.decode()


@pytest.fixture(scope="module")
def emu_kit(tmp_path_factory, emu_lib):
    return Kit(os.path.join(ROOT, "tests", "emu", "bamkit_emu"), os.path.join(ROOT, "tests", "emu", "sambamba_emu"), tmp_path_factory.mktemp("b2f_emu"))


@pytest.fixture(scope="module")
def gpu_kit(tmp_path_factory, gpu_lib):
    return Kit(os.path.join(ROOT, "bin", "bamkit"), os.path.join(ROOT, "bin", "sambamba"), tmp_path_factory.mktemp("b2f_gpu"))


DEV = {"SSG_B2F_DEVICE": "1"}
CLI = {   # args, the files, the model's arguments, more environment, the least number of batches
    "plain": ([], ("a",), {}, {}, 1),
    "read_groups": (["-r", "gb,gc"], ("a",), dict(rg=("gb", "gc")), {}, 1),
    "rename": (["-n"], ("a",), dict(rename=True), {}, 1),
    "two_files": ([], ("a", "b"), {}, {}, 2),
    "two_files_renamed": (["-n", "-r", "ga"], ("b", "a"), dict(rg=("ga",), rename=True), {}, 2),
    "small_batches": ([], ("a",), {}, {"SSG_B2F_BATCH": "20000"}, 8),
}


def check_cli(kit, name):
    args, files, model, extra, least = CLI[name]
    paths = [kit.path(f) for f in files]
    rc, host, err_host = kit.run(args + paths, {})
    assert rc == 0 and "on the device" not in err_host
    want, left = ref.fastq_of_files([kit.plain(f) for f in files], **model)
    assert host == want, first_difference(host, want)
    assert len(want) > 100000 and left > 10 and "%d reads without their mate" % left in err_host
    rc, dev, err = kit.run(args + paths, dict(DEV, **extra))
    assert rc == 0, err[-2000:]
    m = re.search(r"bamtofastq: on the device: (\d+) files?, (\d+) members, (\d+) records scanned, (\d+) pairs, (\d+) halves left, (\d+) batch", err)
    assert m, err[-2000:]
    assert dev == host, first_difference(dev, host)
    n_rec = sum(len(ref.split_records(kit.plain(f), ref.bam_records(kit.plain(f)))) for f in files)
    assert (int(m.group(1)), int(m.group(3)), int(m.group(4)), int(m.group(5))) == (len(files), n_rec, want.count(b"\n") // 8, left) and int(m.group(6)) >= least
    assert "%d reads without their mate" % left in err


@pytest.mark.parametrize("name", sorted(CLI))
def test_emu_bamtofastq_device_writes_the_host_text(emu_kit, name):
    check_cli(emu_kit, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CLI))
def test_gpu_bamtofastq_device_writes_the_host_text(gpu_kit, name):
    check_cli(gpu_kit, name)


def check_cli_fallbacks(kit):
    rc, host, _ = kit.run([kit.path("a")], {})
    assert rc == 0
    rc, out, err = kit.run([kit.path("skew")], DEV)                         # blocks that split records: a property of the file
    assert rc == 0 and out == host and "on the device" not in err and re.search(r"bamtofastq: on the host: .*not record-aligned", err), err[-2000:]
    with open(kit.path("a"), "rb") as f:
        p = subprocess.Popen(["cat"], stdin=f, stdout=subprocess.PIPE)
        rc, out, err = kit.run(["/dev/stdin"], DEV, stdin=p.stdout)
        p.wait()
    assert rc == 0 and out == host and re.search(r"bamtofastq: on the host: .*not a regular file", err), err[-2000:]
    rc, out, err = kit.run([kit.path("a")], dict(DEV, SSG_B2F_POOL="10000"))                                                        # a store too small for one batch
    assert rc == 0 and out == host and re.search(r"bamtofastq: on the host: .*capacity", err), err[-2000:]
    rc, out, err = kit.run([kit.path("a")], {"SSG_B2F_DEVICE": "0"})
    assert rc == 0 and out == host and "on the device" not in err and "on the host" not in err


def test_emu_bamtofastq_fallbacks(emu_kit):
    check_cli_fallbacks(emu_kit)


@pytest.mark.gpu
def test_gpu_bamtofastq_fallbacks(gpu_kit):
    check_cli_fallbacks(gpu_kit)
