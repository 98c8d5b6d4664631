"""Picard's duplicate rule on the device (k_markdup.h; ssg_markdup_*): the duplicate set, the eight counts and the bytes behind the second pass against
tests/markdup_reference.py -- a model that shares no code with the product: dicts keyed by tuples, names as bytes, nothing hashed, packed or sorted -- at every
wave and workgroup edge of every kernel, with groups that span waves, workgroups and pushes, on every form of the key and the score, through the mate join's
corners, and every refusal by its code and words.  CPU-side on the host emulation of the kernels; `-m gpu' on the MI355X."""
import functools
import struct

import numpy as np
import pytest

import markdup_reference as model
import view_reference as ref
from speedseq_amd import capi
from test_bam_scan import make_member, rec
from test_bam_select import COUNTS
from test_bgzf_inflate import concat
from test_stats import srec

SSG_EIO, SSG_ENOMEM, SSG_EINVAL, SSG_ERANGE, SSG_EALIGN, SSG_EOVERFLOW = -5, -12, -22, -34, -71, -75
M, I, D, N, S, H, P, EQ, X = range(9)
AB64 = 0xABABABABABABABAB
KINDS = ("stored", "fixed", "dynamic")
P1, P2 = 0x1 | 0x40 | 0x20, 0x1 | 0x80 | 0x10          # a forward first mate and its reverse second mate


def err(lib):
    return lib.l.ssg_last_error().decode()


def mk(name, flag=0, tid=0, pos=100, cigar=((10, M),), qual=(30, 30, 30, 30), rg=None, extra=b""):
    """one record: these quality bytes, an RG:Z tag if given"""
    aux = (b"RGZ" + rg + b"\0" if rg is not None else b"") + extra
    return srec(tid, pos, flag, list(cigar), [1] * len(qual), list(qual), name=name + b"\0", extra=aux)


def pair(name, pos1=100, pos2=300, q1=(30,) * 4, q2=(30,) * 4, tid1=0, tid2=0, f1=P1, f2=P2, **kw):
    """a forward first mate at pos1 and a reverse second mate that begins at pos2"""
    return [mk(name, f1, tid1, pos1, qual=q1, **kw), mk(name, f2, tid2, pos2, qual=q2, **kw)]


def members(records, sizes=(40, 7, 64)):
    """the records as members' payloads of 40, 7, 64, ... records: every member begins at a record"""
    out, i, k = [], 0, 0
    while i < len(records):
        out.append(b"".join(records[i:i + sizes[k % len(sizes)]]))
        i += sizes[k % len(sizes)]
        k += 1
    return out


def append(lib, recs, records):
    blob, moff = concat([make_member(p, KINDS[k % 3]) for k, p in enumerate(members(records))])
    rc, cid, off, st = capi.recs_append_bgzf(lib, recs, blob, moff)
    assert rc == 0 and (st == 0).all(), err(lib)
    return cid, off


def second_pass(lib, recs, m, chunks, remove):
    """the chunks appended again and applied; (the gathered bytes, the flags of the entries that came back)"""
    out, flags = [], []
    for c in chunks:
        if not c:
            continue
        cid, off = append(lib, recs, c)
        rc, n_rec, n_kept, loc, ent = capi.markdup_apply(lib, m, cid, off, remove=remove)
        assert rc == 0 and n_rec == len(c), err(lib)
        cum = np.zeros(n_kept + 1, dtype=np.uint64)
        cum[1:] = np.cumsum(ent["len"].astype(np.uint64))
        capi.recs_order(lib, recs, loc, cum)
        out.append(capi.recs_gather(lib, recs, 0, int(cum[-1])).tobytes() if n_kept else b"")
        capi.recs_reopen(lib, recs)
        capi.recs_release(lib, recs, cid)
        flags += [int(f) for f in ent["flag"]]
    return b"".join(out), flags


def flow(lib, chunks, rg=(), libs=(), hash_bits=64, remove=False):
    """the chunks (lists of records) pushed in order, decided, and passed again; (duplicate ordinals, counts, the bytes behind the second pass, the entries' flags)"""
    recs = capi.recs_create(lib, 1 << 40)
    rc, m = capi.markdup_create(lib, recs, rg, libs, hash_bits)
    assert rc == 0, err(lib)
    n = 0
    for c in chunks:
        if not c:
            continue
        cid, off = append(lib, recs, c)
        rc, n_rec = capi.markdup_push(lib, m, cid, off)
        assert rc == 0 and n_rec == len(c), err(lib)
        n += n_rec
    rc, counts = capi.markdup_finish(lib, m)
    assert rc == 0, err(lib)
    rc, dup = capi.markdup_get(lib, m, 0, n)
    assert rc == 0 and set(np.unique(dup)) <= {0, 1}, err(lib)
    data, flags = second_pass(lib, recs, m, chunks, remove)
    m.close(); recs.close()
    return set(int(i) for i in np.nonzero(dup)[0]), counts, data, flags


def check(lib, chunks, rg=(), libs=(), hash_bits=64, modes=(False,)):
    """flow(), and the duplicates, the counts and the bytes are the model's; returns (duplicates, counts)"""
    if chunks and isinstance(chunks[0], bytes):
        chunks = [chunks]
    stream = ref.records(b"".join(r for c in chunks for r in c), 0)
    want, want_counts = model.compute(stream, rg, libs)
    for remove in modes:
        got, counts, data, flags = flow(lib, chunks, rg, libs, hash_bits, remove)
        assert got == want, (sorted(got - want)[:10], sorted(want - got)[:10])
        assert counts == want_counts
        exp = model.expected_bytes(stream, want, remove)
        assert data == b"".join(exp)
        assert flags == [struct.unpack_from("<H", b, 18)[0] for b in exp]
    return want, want_counts


# ---- wave and workgroup edges of every kernel: one group, distinct groups, groups of two; fragments and pairs; both modes ----
def n_of(name):
    return 10243 if name.startswith("members_") else int(name)


@functools.lru_cache(maxsize=None)
def edge_records(name, layout, kind):
    n, out = n_of(name), []
    site = {"one": lambda k: 0, "distinct": lambda k: k, "twos": lambda k: k // 2}[layout]
    for k in range(n if kind == "frag" else n // 2):
        q = (20 + (k * 7) % 23,) * (1 + k % 3)
        if kind == "frag":
            out.append(mk(b"f%d" % k, 0x10 if k % 5 == 0 and layout != "one" else 0, pos=1000 + 3 * site(k), qual=q))
        else:
            out += pair(b"p%d" % k, 1000 + 3 * site(k), 5000 + 3 * site(k), q1=q)
    if kind == "pair" and n % 2:
        out.append(mk(b"odd", 0, pos=77))
    return out


def check_edges(lib, name):
    for layout in ("one", "distinct", "twos"):
        for kind in ("frag", "pair"):
            records = edge_records(name, layout, kind)
            dup, counts = check(lib, records, modes=(False, True) if kind == "frag" or n_of(name) < 1000 else (True,))
            assert counts["records"] == n_of(name)
            if kind == "frag" and layout == "distinct":
                assert not dup
            if kind == "frag" and layout == "one":
                assert len(dup) == n_of(name) - 1
    if name == "1":
        assert check(lib, [])[1]["records"] == 0


@pytest.mark.parametrize("name", COUNTS)
def test_emu_markdup_wave_and_workgroup_edges(emu_lib, name):
    check_edges(emu_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", COUNTS)
def test_gpu_markdup_wave_and_workgroup_edges(gpu_lib, name):
    check_edges(gpu_lib, name)


# ---- groups across waves, workgroups and launch edges: the best member first, last, at 63 / 64, at 255 / 256; all equal; split over three pushes ----
GROUP_SIZES = (300, 1025, 5000)


@functools.lru_cache(maxsize=None)
def group_records(size, tie):
    """per place of the best member one fragment group and one pair group of `size' members, every group at a site of its own"""
    out = []
    places = (0,) if tie else (0, 63, 64, 255, 256, size - 1)
    for g, best in enumerate(places):
        for k in range(size):
            q = (30,) if tie else ((40,) if k == best else (20 + k % 7,))
            out.append(mk(b"f%d_%d" % (g, k), 0, pos=1000 + g, qual=q))
            out += pair(b"p%d_%d" % (g, k), 20000 + g, 30000 + g, q1=q, q2=(25,))
    return out


def check_groups(lib, size):
    for tie in (False, True):
        records = group_records(size, tie)
        places = (0,) if tie else (0, 63, 64, 255, 256, size - 1)
        dup, counts = check(lib, records)
        assert len(dup) == len(records) - 3 * len(places)
        for g, best in enumerate(places):                               # the best of every group is what is left of it
            base = 3 * (g * size + best)
            assert not {base, base + 1, base + 2} & dup
    if size == GROUP_SIZES[0]:                                          # a group split over three pushes
        records = group_records(size, False)
        a, b = len(records) // 3 + 1, 2 * len(records) // 3 + 2
        check(lib, [records[:a], records[a:b], records[b:]])
        check(lib, [records[:5], [], records[5:b], records[b:]], modes=(True,))


@pytest.mark.parametrize("size", GROUP_SIZES)
def test_emu_markdup_groups_across_edges(emu_lib, size):
    check_groups(emu_lib, size)


@pytest.mark.gpu
@pytest.mark.parametrize("size", GROUP_SIZES)
def test_gpu_markdup_groups_across_edges(gpu_lib, size):
    check_groups(gpu_lib, size)


# ---- the key ----
BIG = (1 << 28) - 1


def key_records():
    out = []
    def two(name, a, b):                                                # two fragments: duplicates of each other exactly when their keys are equal
        out.append(mk(name + b"a", **a)); out.append(mk(name + b"b", **b))
    # leading S, H and S+H runs on the forward strand: 100 - 7 = 93
    two(b"ls", dict(pos=100, cigar=((7, S), (10, M))), dict(pos=93, cigar=((10, M),)))
    two(b"lh", dict(pos=200, cigar=((7, H), (10, M))), dict(pos=193, cigar=((10, M),)))
    two(b"lhs", dict(pos=300, cigar=((3, H), (4, S), (10, M))), dict(pos=293, cigar=((10, M), (9, S))))
    two(b"lsx", dict(pos=400, cigar=((7, S), (10, M))), dict(pos=400, cigar=((10, M),)))                       # (not equal)
    # trailing runs on the reverse strand: end - 1 + clips
    two(b"ts", dict(flag=16, pos=500, cigar=((10, M), (7, S))), dict(flag=16, pos=507, cigar=((10, M),)))
    two(b"th", dict(flag=16, pos=600, cigar=((10, M), (7, H))), dict(flag=16, pos=607, cigar=((3, S), (10, M),)))
    two(b"tsh", dict(flag=16, pos=700, cigar=((10, M), (4, S), (3, H))), dict(flag=16, pos=702, cigar=((15, M),)))
    two(b"mid", dict(pos=800, cigar=((2, S), (5, M), (3, I), (5, M))), dict(pos=798, cigar=((13, M),)))     # an insertion ends the leading run
    # u5 < 0 and u5 > 2^31
    two(b"neg", dict(pos=3, cigar=((10, S), (5, M))), dict(pos=1, cigar=((8, S), (5, M))))
    two(b"neg2", dict(pos=3, cigar=((12, S), (5, M))), dict(pos=3, cigar=((11, S), (5, M))))
    top = (1 << 31) - 200
    two(b"big", dict(flag=16, pos=top, cigar=((100, M), (BIG, S), (BIG, H))), dict(flag=16, pos=top + 50, cigar=((50, M), (BIG, H), (BIG, S))))
    two(b"big2", dict(flag=16, pos=top, cigar=((100, M), (BIG, S))), dict(flag=16, pos=top, cigar=((100, M), (BIG - 1, S))))
    # D and N in the reference span
    two(b"dn", dict(flag=16, pos=900, cigar=((5, M), (3, D), (5, M), (100, N), (5, M))), dict(flag=16, pos=900, cigar=((118, M),)))
    two(b"dn2", dict(flag=16, pos=1200, cigar=((5, M), (3, I), (5, M), (2, P))), dict(flag=16, pos=1200, cigar=((10, M),)))
    # a CIGAR of clips only: both runs are the whole of it
    two(b"clipf", dict(pos=1500, cigar=((4, S), (2, H))), dict(pos=1494, cigar=((5, M),)))
    two(b"clipr", dict(flag=16, pos=1600, cigar=((4, S), (2, H))), dict(flag=16, pos=1596, cigar=((10, M),)))
    # equal (tid, u5), opposite strands: different fragment keys
    two(b"opp", dict(pos=1700, cigar=((10, M),)), dict(flag=16, pos=1691, cigar=((10, M),)))
    two(b"tid", dict(tid=1, pos=1800), dict(tid=2, pos=1800))
    # the pair key orders the forward end first: an RF pair and the FR pair of the same ends
    out.extend(pair(b"fr", 2000, 1991, f1=0x1 | 0x40 | 0x20, f2=0x1 | 0x80 | 0x10))                          # forward at u5 2000, reverse at u5 2000
    out.extend([mk(b"rf", 0x1 | 0x40 | 0x10, 0, 1991), mk(b"rf", 0x1 | 0x80 | 0x20, 0, 2000)])
    # two pairs that differ only in which mate has 0x40
    out.extend(pair(b"m40a", 2200, 2400))
    out.extend(pair(b"m40b", 2200, 2400, f1=0x1 | 0x80 | 0x20, f2=0x1 | 0x40 | 0x10))
    # the ends of a pair on two contigs, in both orders in the stream
    out.extend(pair(b"x1", 2600, 2700, tid1=1, tid2=0))
    out.extend([mk(b"x2", P2, 0, 2700), mk(b"x2", P1, 1, 2600)])
    return out


def check_key(lib):
    records = key_records()
    dup, _ = check(lib, records, modes=(False, True))
    names = [r["name"] for r in ref.records(b"".join(records), 0)]
    marked = sorted(set(names[o][:-1] if names[o][-1:] in b"ab" and not names[o].startswith((b"m40", b"x", b"fr", b"rf")) else names[o] for o in dup))
    assert marked == sorted([b"ls", b"lh", b"lhs", b"ts", b"th", b"tsh", b"mid", b"neg", b"big", b"dn", b"dn2", b"clipf", b"clipr", b"rf", b"m40b", b"x2"])
    assert sum(1 for o in dup if names[o] == b"rf") == 2 and sum(1 for o in dup if names[o] == b"x2") == 2


def test_emu_markdup_key(emu_lib):
    check_key(emu_lib)


@pytest.mark.gpu
def test_gpu_markdup_key(gpu_lib):
    check_key(gpu_lib)


def library_records():
    out = [mk(b"a1", pos=100, rg=b"g1", qual=(40,)), mk(b"a2", pos=100, rg=b"g2", qual=(30,)),                # g1, g2: library 1 -- one group
           mk(b"b1", pos=100, rg=b"g3", qual=(20,)),                                                          # g3: library 2 -- another
           mk(b"c1", pos=100, qual=(20,)), mk(b"c2", pos=100, rg=b"nobody", qual=(21,)), mk(b"c3", pos=100, rg=b"g4", qual=(22,)),   # none, unknown, an @RG without LB: library 0
           mk(b"d1", pos=100, rg=b"g1x", qual=(50,)), mk(b"d2", pos=100, rg=b"g", qual=(50,)),                # a longer and a shorter id are unknown
           mk(b"e1", pos=100, extra=b"RGZg3\0XAi\1\0\0\0RGZg1\0", qual=(10,)),                                # the last RG:Z counts: library 1
           mk(b"e2", pos=100, extra=b"XBBs\2\0\0\0\1\0\2\0RGZg3\0", qual=(19,)),                              # behind a B array: library 2
           mk(b"e3", pos=100, extra=b"RGZg3\0XDd" + bytes(8) + b"RGZg1\0", qual=(18,))]                       # the walk ends at the unknown type: library 2
    out += pair(b"p1", 700, 900, rg=b"g1") + pair(b"p2", 700, 900, rg=b"g2") + pair(b"p3", 700, 900, rg=b"g3")
    return out


def check_libraries(lib):
    records = library_records()
    dup, _ = check(lib, records, rg=(b"g1", b"g2", b"g3", b"g4"), libs=(1, 1, 2, 0), modes=(False, True))
    names = [r["name"] for r in ref.records(b"".join(records), 0)]
    assert sorted(set(names[o] for o in dup)) == [b"a2", b"c1", b"c2", b"c3", b"d2", b"e1", b"e2", b"e3", b"p2"]
    dup, _ = check(lib, records)                                         # without a list every record is of library 0
    assert len(dup) == 10 + 4


def test_emu_markdup_libraries(emu_lib):
    check_libraries(emu_lib)


@pytest.mark.gpu
def test_gpu_markdup_libraries(gpu_lib):
    check_libraries(gpu_lib)


# ---- the score ----
def check_score(lib):
    out = [mk(b"q14", pos=100, qual=(14,) * 30), mk(b"q15", pos=100, qual=(15,)),                             # 0 against 15
           mk(b"ff", pos=200, qual=(0xff,)), mk(b"fe", pos=200, qual=(0xfe,)), mk(b"lo", pos=200, qual=(127, 127)),   # 255 > 254 = 254: unsigned bytes
           mk(b"z0", pos=300, qual=()), mk(b"z1", pos=300, qual=(14,)), mk(b"z2", pos=300, qual=(15,))]       # l_seq == 0 scores 0: the first of the zeros loses to 15
    out += [mk(b"odd%d" % k, pos=400, qual=(16,) * k) for k in (1, 2, 3, 4, 5, 63, 64, 65, 67, 129, 66)]      # every alignment of the qualities, every tail
    # a pair that wins on the sum though each of its ends loses
    out += pair(b"w1", 600, 800, q1=(40,), q2=(15,)) + pair(b"w2", 600, 800, q1=(15,), q2=(41,)) + pair(b"w3", 600, 800, q1=(39,), q2=(39,))
    dup, _ = check(lib, out, modes=(False, True))
    names = [r["name"] for r in ref.records(b"".join(out), 0)]
    kept = set(names) - set(names[o] for o in dup)
    assert kept == {b"q15", b"ff", b"z2", b"odd129", b"w3"}


def test_emu_markdup_score(emu_lib):
    check_score(emu_lib)


@pytest.mark.gpu
def test_gpu_markdup_score(gpu_lib):
    check_score(gpu_lib)


def check_saturation(lib):
    """one record of 5 M bases of quality 0xff takes the sum past 2^30: it ties with a second such record (the smaller ordinal wins) where an unsaturated sum
    of 5000001 * 255 would have won; a record too long for a BGZF member lies across members, so the hints are the stream's two ends"""
    n = 5000000
    big = [rec(0, 100, 0, [(10, M)], name=b"s%d\0" % k, l_seq=n + k) for k in range(2)]
    big = [b[:36 + 3 + 4 + (n + k + 1) // 2] + b"\xff" * (n + k) for k, b in enumerate(big)]
    small = mk(b"t", pos=100, qual=(0xff,) * 100)
    stream = b"".join(big) + small
    recs = capi.recs_create(lib, 1 << 40)
    rc, m = capi.markdup_create(lib, recs)
    assert rc == 0
    blob, moff = concat([make_member(stream[o:o + 0xff00], "stored") for o in range(0, len(stream), 0xff00)])
    rc, cid, off, st = capi.recs_append_bgzf(lib, recs, blob, moff)
    assert rc == 0 and int(off[-1]) == len(stream)
    rc, n_rec = capi.markdup_push(lib, m, cid, [0, len(stream)])
    assert (rc, n_rec) == (0, 3), err(lib)
    rc, counts = capi.markdup_finish(lib, m)
    rc, dup = capi.markdup_get(lib, m, 0, 3)
    assert rc == 0 and list(dup) == [0, 1, 1] and counts["dup_fragments"] == 2
    want, _ = model.compute(ref.records(stream, 0))
    assert want == {1, 2}
    m.close(); recs.close()


def test_emu_markdup_saturation(emu_lib):
    check_saturation(emu_lib)


@pytest.mark.gpu
def test_gpu_markdup_saturation(gpu_lib):
    check_saturation(gpu_lib)


# ---- the mate join ----
def join_records():
    out = []
    out += [mk(b"far", P1, 0, 100)] + [mk(b"fill%d" % k, 0, 1, 10 * k) for k in range(4000)] + [mk(b"far", P2, 1, 900)]   # mates on two contigs, 4000 records apart
    out += pair(b"far2", 100, 900, tid2=1)                                                                     # the same ends: a duplicate pair
    # three and four records of one name: a same-0xc0 record is ignored, then the pair forms
    out += [mk(b"tri", P1, 0, 3000), mk(b"tri", P1 | 0x400, 0, 3050), mk(b"tri", P2, 0, 3200)]
    out += pair(b"tri2", 3000, 3200)
    out += [mk(b"quad", P1, 0, 3400), mk(b"quad", P2, 0, 3600), mk(b"quad", P2, 0, 3700), mk(b"quad", P1, 0, 3800)]   # two pairs of one name
    out += pair(b"quad2", 3800, 3700)
    # a paired record whose mate does not take part: secondary, unmapped, absent.  It is never marked and makes the fragments at its key duplicates
    out += [mk(b"sec", P1, 0, 5000), mk(b"sec", P2 | 0x100, 0, 5200), mk(b"secf", 0, 0, 5000, qual=(60,) * 9)]
    out += [mk(b"unm", P1, 0, 5400), mk(b"unm", 0x1 | 0x80 | 0x4, 0, 5400), mk(b"unmf", 0, 0, 5400)]
    out += [mk(b"abs", P1, 0, 5600), mk(b"absf1", 0, 0, 5600), mk(b"absf2", 0, 0, 5600), mk(b"abs_other", P1, 0, 5600)]
    out += [mk(b"mu", 0x1 | 0x8 | 0x40, 0, 5800, qual=(20,)), mk(b"muf", 0, 0, 5800, qual=(30,))]              # 0x8: a fragment by its flags
    # names of every length, names that differ in their last byte only, one the prefix of another
    for k, nm in enumerate((b"n", b"nn", b"nn" * 60, b"nn" * 60 + b"x", b"nn" * 60 + b"y", b"n" * 254)):
        out += pair(nm, 7000 + k, 7500 + k)
    return out


def check_join(lib):
    records = join_records()
    results = [check(lib, records, hash_bits=hb, modes=(False, True) if hb == 64 else (False,)) for hb in (64, 3)]
    records = [r for r in records if b"fill" not in r[36:41]] + [mk(b"fill%d" % k, 0, 1, 10 * k) for k in range(40)]
    results.append(check(lib, records, hash_bits=0))                     # (one run: at most 256 paired records)
    dup, counts = results[0]
    names = [r["name"] for r in ref.records(b"".join(join_records()), 0)]
    marked = sorted(set(names[o] for o in dup))
    assert marked == sorted([b"far2", b"tri2", b"quad2", b"secf", b"unmf", b"absf1", b"absf2", b"mu"])
    assert counts["unmatched"] == 1 + 1 + 1 + 2 and counts["pairs"] == 2 + 2 + 3 + 6
    # mates in different pushes
    a = records.index(mk(b"tri", P2, 0, 3200))
    check(lib, [records[:a], records[a:]], hash_bits=3)


def test_emu_markdup_mate_join(emu_lib):
    check_join(emu_lib)


@pytest.mark.gpu
def test_gpu_markdup_mate_join(gpu_lib):
    check_join(gpu_lib)


def check_run_max(lib):
    """257 paired records in one run are SSG_ERANGE and the object is as before: it still takes pushes, refuses get, and is freed; 256 are decided"""
    for n, want in ((capi.MARKDUP_RUN_MAX, 0), (capi.MARKDUP_RUN_MAX + 1, SSG_ERANGE)):
        records = [mk(b"r%d" % k, P1, 0, 10 * k) for k in range(n)] + [mk(b"f", 0, 0, 5)]
        recs = capi.recs_create(lib, 1 << 40)
        rc, m = capi.markdup_create(lib, recs, hash_bits=0)
        cid, off = append(lib, recs, records)
        assert capi.markdup_push(lib, m, cid, off) == (0, n + 1)
        rc, counts = capi.markdup_finish(lib, m)
        assert rc == want, err(lib)
        if want:
            assert "more than 256 paired records share one name hash of 0 bits" in err(lib)
            assert capi.markdup_get(lib, m, 0, 1)[0] == SSG_EINVAL
            cid, off = append(lib, recs, [mk(b"g", 0, 0, 5)])
            assert capi.markdup_push(lib, m, cid, off) == (0, 1)
            assert capi.markdup_finish(lib, m)[0] == SSG_ERANGE
        else:
            assert counts["unmatched"] == n and counts["pairs"] == 0
        m.close(); recs.close()


def test_emu_markdup_run_max(emu_lib):
    check_run_max(emu_lib)


@pytest.mark.gpu
def test_gpu_markdup_run_max(gpu_lib):
    check_run_max(gpu_lib)


# ---- records that do not take part; 0x400 that came in ----
def check_not_taking_part(lib):
    out = []
    for k, fl in enumerate((0x4, 0x100, 0x800, 0x4 | 0x400, 0x100 | 0x400, 0x800 | 0x400)):
        out.append(mk(b"np%d" % k, fl, 0, 100))
    out += [rec(0, 100, 0, [], name=b"nc\0", l_seq=4), rec(0, 100, 0x400, [], name=b"ncd\0", l_seq=4)]          # n_cigar == 0
    out += [mk(b"was", 0x400, 0, 100, qual=(50,)), mk(b"is", 0, 0, 100, qual=(40,)), mk(b"lone", 0x400, 0, 900)]  # 0x400 cleared on the kept ones
    out += [mk(b"pw", P1 | 0x400, 0, 2000), mk(b"pw", P2 | 0x400, 0, 2200)]
    dup, counts = check(lib, out, modes=(False, True))
    assert dup == {9} and counts["taking_part"] == 5 and counts["records"] == 13


def test_emu_markdup_not_taking_part(emu_lib):
    check_not_taking_part(emu_lib)


@pytest.mark.gpu
def test_gpu_markdup_not_taking_part(gpu_lib):
    check_not_taking_part(gpu_lib)


# ---- apply: one bit and nothing else; refusals ----
def check_apply(lib):
    records = edge_records("257", "twos", "frag") + edge_records("65", "one", "pair")
    stream = b"".join(records)
    want, _ = model.compute(ref.records(stream, 0))
    for remove in (False, True):
        got, counts, data, flags = flow(lib, [records], remove=remove)
        assert got == want
        if not remove:                                                   # the input under a mask of the one bit
            assert len(data) == len(stream)
            diff = np.frombuffer(data, dtype=np.uint8) ^ np.frombuffer(stream, dtype=np.uint8)
            at = np.nonzero(diff)[0]
            offs = {r["off"] + 19: o for o, r in enumerate(ref.records(stream, 0))}
            assert all(int(a) in offs and diff[a] == 4 for a in at)
            assert {offs[int(a)] for a in at} == want                    # (no record came in with 0x400)
    recs = capi.recs_create(lib, 1 << 40)
    rc, m = capi.markdup_create(lib, recs)
    cid, off = append(lib, recs, records)
    # before finish
    assert capi.markdup_apply(lib, m, cid, off)[0] == SSG_EINVAL and "ssg_markdup_finish first" in err(lib)
    assert capi.markdup_get(lib, m, 0, 0)[0] == SSG_EINVAL and "ssg_markdup_finish first" in err(lib)
    assert capi.markdup_push(lib, m, cid, off) == (0, len(records))
    assert capi.markdup_finish(lib, m)[0] == 0
    n_kept = len(records) - len(want)
    # the counting form: the two numbers, nothing patched, the ordinal stays
    cid, off = append(lib, recs, records)
    assert capi.markdup_apply(lib, m, cid, off, remove=True, counting=True)[:3] == (0, len(records), n_kept)
    assert capi.markdup_apply(lib, m, cid, off, counting=True)[:3] == (0, len(records), len(records))
    # room for one record less
    rc, n_rec, n_k, loc, ent = capi.markdup_apply(lib, m, cid, off, remove=True, cap=n_kept - 1)
    assert (rc, n_rec, n_k) == (SSG_EOVERFLOW, len(records), n_kept) and "records kept, room for" in err(lib)
    assert (loc == AB64).all() and ent.tobytes() == b"\xab" * ent.nbytes
    # no arrays and a capacity
    assert lib.l.ssg_markdup_apply(m.h, cid, None, 0, 0, 0, 5, None, None, None, None) == SSG_EINVAL
    # a changed stream: another name, another block_size
    changed = list(records); changed[70] = mk(b"other", 0, pos=1000 + 3 * 35, qual=(20,) * 2)
    cid2, off2 = append(lib, recs, changed)
    assert capi.markdup_apply(lib, m, cid2, off2)[0] == SSG_EIO and "the stream changed between the passes: the record of ordinal 70 " in err(lib)
    changed = list(records); changed[0] = mk(b"f0", 0, pos=1000, qual=(20,), extra=b"XXA!")
    cid3, off3 = append(lib, recs, changed)
    assert capi.markdup_apply(lib, m, cid3, off3)[0] == SSG_EIO and "ordinal 0 " in err(lib)
    # nothing was patched by the refusals: the chunk gathers as it came
    rc, n_rec, n_k, loc, ent = capi.markdup_apply(lib, m, cid, off, remove=True, cap=n_kept)
    assert (rc, n_rec, n_k) == (0, len(records), n_kept), err(lib)
    assert [int(x) & ((1 << 40) - 1) for x in loc] == [r["off"] for o, r in enumerate(ref.records(stream, 0)) if o not in want]
    # a chunk too many
    cid4, off4 = append(lib, recs, records[:1])
    assert capi.markdup_apply(lib, m, cid4, off4)[0] == SSG_EINVAL and "run past the %d records of the first pass" % len(records) in err(lib)
    assert capi.markdup_get(lib, m, len(records), 1)[0] == SSG_EINVAL
    m.close(); recs.close()


def test_emu_markdup_apply(emu_lib):
    check_apply(emu_lib)


@pytest.mark.gpu
def test_gpu_markdup_apply(gpu_lib):
    check_apply(gpu_lib)


# ---- refusals and state ----
def check_refusals(lib):
    recs = capi.recs_create(lib, 1 << 40)
    for kw, words in ((dict(rg=(None,), lib_of_rg=(1,)), "read group id 0 is NULL or empty"), (dict(rg=(b"a", b""), lib_of_rg=(1, 2)), "read group id 1 is NULL or empty"),
                      (dict(n_rg=-1), "n_rg < 0"), (dict(rg=(b"a",), lib_of_rg=()), "no rg[] / lib_of_rg[]"), (dict(hash_bits=-1), "hash_bits outside 0 .. 64"),
                      (dict(hash_bits=65), "hash_bits outside 0 .. 64")):
        rc, m = capi.markdup_create(lib, recs, **kw)
        assert rc == SSG_EINVAL and words in err(lib), (kw, err(lib))
    assert capi.markdup_create(lib, None)[0] == SSG_EINVAL and "no record store" in err(lib)
    rc, m = capi.markdup_create(lib, recs)
    assert rc == 0
    # a bad stream in the scan's words
    good = [mk(b"a", pos=5), mk(b"b", pos=6)]
    blob, moff = concat([make_member(good[0] + good[1][:20], "fixed"), make_member(good[1][20:] + good[0], "stored")])
    rc, cid, off, st = capi.recs_append_bgzf(lib, recs, blob, moff)
    assert capi.markdup_push(lib, m, cid, off)[0] == SSG_EALIGN and err(lib).startswith("ssg_markdup_push: ")
    assert capi.markdup_push(lib, m, cid, [0, int(off[-1])]) == (0, 3)   # (the same chunk, repeated with other hints)
    bad = bytearray(good[0]); struct.pack_into("<I", bad, 0, 20)
    cid, off = append(lib, recs, [bytes(bad)])
    assert capi.markdup_push(lib, m, cid, off)[0] == SSG_EIO and err(lib).startswith("ssg_markdup_push: ")
    assert capi.markdup_push(lib, m, 99, off)[0] == SSG_EINVAL and err(lib).startswith("ssg_markdup_push: ")
    bad = bytearray(mk(b"long", pos=5)); struct.pack_into("<i", bad, 20, 400)                                  # l_seq beyond block_size
    cid, off = append(lib, recs, [good[0], bytes(bad)])
    assert capi.markdup_push(lib, m, cid, off)[0] == SSG_EIO and "malformed record at offset %d: 32 + l_qname + 4 n_cigar" % len(good[0]) in err(lib)
    # while an order is declared
    cid, off = append(lib, recs, good)
    capi.recs_order(lib, recs, np.array([cid << 40], dtype=np.uint64), np.array([0, len(good[0])], dtype=np.uint64))
    assert capi.markdup_push(lib, m, cid, off)[0] == SSG_EINVAL and "refused while an order is declared" in err(lib)
    capi.recs_reopen(lib, recs)
    assert capi.markdup_push(lib, m, cid, off) == (0, 2)
    rc, counts = capi.markdup_finish(lib, m)
    assert rc == 0 and counts["records"] == 5 and counts["dup_fragments"] == 3
    # after finish
    cid, off = append(lib, recs, good)
    assert capi.markdup_push(lib, m, cid, off)[0] == SSG_EINVAL and "the object is finished" in err(lib)
    assert capi.markdup_finish(lib, m)[0] == SSG_EINVAL and "finished already" in err(lib)
    m.close(); recs.close()


def test_emu_markdup_refusals_and_state(emu_lib):
    check_refusals(emu_lib)


@pytest.mark.gpu
def test_gpu_markdup_refusals_and_state(gpu_lib):
    check_refusals(gpu_lib)


def check_capacity(lib):
    """the entries count against the store's capacity: SSG_ENOMEM with everything as before, and the push goes through once something else is released"""
    records = [mk(b"c%d" % k, 0, 0, 100 + k % 50) for k in range(2000)] + pair(b"pp", 5, 500) * 100
    payload = sum(len(r) for r in records)
    recs = capi.recs_create(lib, 2 * payload + 2200 * 40 // 2)
    rc, m = capi.markdup_create(lib, recs)
    other, _ = append(lib, recs, records)
    cid, off = append(lib, recs, records)
    assert capi.markdup_push(lib, m, cid, off)[0] == SSG_ENOMEM and "store's capacity" in err(lib)
    rc, n, _, _, _ = capi.recs_scan(lib, recs, cid, off)                 # the chunk is still there
    assert (rc, n) == (0, len(records))
    capi.recs_release(lib, recs, other)
    assert capi.markdup_push(lib, m, cid, off) == (0, len(records))
    rc, counts = capi.markdup_finish(lib, m)
    want, want_counts = model.compute(ref.records(b"".join(records), 0))
    assert rc == 0 and counts == want_counts
    rc, dup = capi.markdup_get(lib, m, 0, len(records))
    assert set(int(i) for i in np.nonzero(dup)[0]) == want
    m.close(); recs.close()


def test_emu_markdup_capacity(emu_lib):
    check_capacity(emu_lib)


@pytest.mark.gpu
def test_gpu_markdup_capacity(gpu_lib):
    check_capacity(gpu_lib)


# ---- seeded random streams ----
READ_LENGTHS = (1, 36, 100, 150, 151)


@functools.lru_cache(maxsize=None)
def random_pairs(seed, n_pairs):
    """n_pairs templates over two contigs, positions from a few dozen sites so that groups form: complete pairs, mates on two contigs, mates that are unmapped,
    secondary or absent, fragments, clips on both strands, three read groups of two libraries; in generation order"""
    rng = np.random.RandomState(seed)
    sites = [(int(rng.randint(2)), int(rng.randint(50, 50000))) for _ in range(40)]
    out = []
    for k in range(n_pairs):
        name = b"t%d" % (k if rng.randint(50) else max(k - 1, 0))        # now and then a name comes twice
        rg = (None, b"A", b"B", b"C")[rng.randint(4)]
        ends = []
        for e in range(2):
            at = int(rng.randint(len(sites))) if e == 0 or rng.randint(2) else (at + 1) % len(sites)   # half of the second ends follow their first end's site
            tid, site = sites[at]
            l = READ_LENGTHS[rng.randint(len(READ_LENGTHS))]
            clip = int(rng.choice([0, 0, 0, 3, 10]))
            rev = int(rng.randint(2))
            cig = [(l, M)] if not clip or clip >= l else ([(l - clip, M), (clip, S)] if rng.randint(2) else [(clip, S), (l - clip, M)])
            pos = site - (clip if cig[0][1] == S and rng.randint(4) else 0) + (0 if rng.randint(10) else int(rng.randint(3)))
            q = rng.choice([2, 14, 15, 30, 41], size=l).astype(np.uint8) if rng.randint(3) else np.full(l, 30, dtype=np.uint8)
            ends.append((tid, pos, rev, cig, bytes(q)))
        what = rng.randint(20)
        for e, (tid, pos, rev, cig, q) in enumerate(ends):
            flag = 0x1 | (0x40, 0x80)[e] | (0x10 if rev else 0) | (0x20 if ends[1 - e][2] else 0)
            if what == 0:                                                # a fragment
                if e: continue
                flag = 0x10 if rev else 0
            elif what == 1 and e:                                        # the mate is unmapped
                flag |= 0x4
            elif what == 1:
                flag |= 0x8
            elif what == 2 and e:                                        # the mate is secondary
                flag |= 0x100
            elif what == 3 and e:                                        # the mate is absent
                continue
            elif what == 4 and e:                                        # a supplementary line behind the pair
                out.append(mk(name, flag | 0x800, tid, pos + 7, cig, q, rg))
            out.append(mk(name, flag | (0x400 if rng.randint(7) == 0 else 0), tid, pos, cig, q, rg))
    return out


def check_random(lib, seed):
    records = random_pairs(seed, 3000)
    rg, libs = (b"A", b"B", b"C"), (1, 2, 1)
    dup, counts = check(lib, records, rg, libs, modes=(False, True))
    assert counts["dup_paired"] > 100 and counts["dup_fragments"] > 20 and counts["unmatched"] > 100
    n = len(records)
    check(lib, [records[:1], records[1:n // 3], records[n // 3:n - 1], records[n - 1:]], rg, libs, hash_bits=11)
    order = sorted(range(n), key=lambda o: (struct.unpack_from("<i", records[o], 4)[0], struct.unpack_from("<i", records[o], 8)[0]))   # coordinate-sorted
    check(lib, [[records[o] for o in order[:n // 2]], [records[o] for o in order[n // 2:]]], rg, libs, modes=(True,))


@pytest.mark.parametrize("seed", (1, 2))
def test_emu_markdup_random_streams(emu_lib, seed):
    check_random(emu_lib, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", (1, 2))
def test_gpu_markdup_random_streams(gpu_lib, seed):
    check_random(gpu_lib, seed)
