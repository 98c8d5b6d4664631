"""The reference of tests/test_markdup.py: Picard's duplicate rule as include/ssgpu.h states it, in plain Python over view_reference.records.  It shares no code
with the product: records are decoded with struct, groups are dicts keyed by tuples, names are bytes, nothing is hashed, packed or sorted.  compute() returns the
set of duplicate ordinals and the eight counts."""
import struct

COUNTS = ("records", "taking_part", "paired", "pairs", "unmatched", "fragments", "dup_paired", "dup_fragments")
CLIPS = (4, 5)
REF_CONSUMING = (0, 2, 3, 7, 8)
SCORE_MAX = (1 << 30) - 1
AUX_SIZES = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}


def last_rg(body, a):
    """the last RG:Z of the aux area that begins at body[a], walked as bamtofastq walks it: an unknown type, a Z / H without its NUL or a B without its five
    bytes end the walk"""
    rg, e = None, len(body)
    while a + 3 <= e:
        tag, ty = body[a:a + 2], body[a + 2:a + 3]
        a += 3
        if ty in AUX_SIZES:
            a += AUX_SIZES[ty]
        elif ty in (b"Z", b"H"):
            q = body.find(b"\0", a)
            if q < 0:
                break
            if tag == b"RG" and ty == b"Z":
                rg = body[a:q]
            a = q + 1
        elif ty == b"B":
            if a + 5 > e:
                break
            cnt, = struct.unpack_from("<I", body, a + 1)
            a += 5 + {b"c": 1, b"C": 1, b"s": 2, b"S": 2}.get(body[a:a + 1], 4) * cnt
        else:
            break
    return rg


def facts(r, lib_of):
    """what the rule reads of one record of view_reference.records"""
    b = r["bytes"]
    l_qname, nc, l = b[12], struct.unpack_from("<H", b, 16)[0], r["l_seq"]
    flag = r["flag"]
    f = {"taking": not (flag & 0x904) and nc > 0, "flag": flag, "name": r["name"]}
    if not f["taking"]:
        return f
    ops = [(v & 0xf, v >> 4) for v in struct.unpack_from("<%dI" % nc, b, 36 + l_qname)]
    lead = 0
    for op, n in ops:
        if op not in CLIPS:
            break
        lead += n
    trail = 0
    for op, n in reversed(ops):
        if op not in CLIPS:
            break
        trail += n
    end = r["pos"] + sum(n for op, n in ops if op in REF_CONSUMING)
    rev = flag >> 4 & 1
    q0 = 36 + l_qname + 4 * nc + (l + 1) // 2
    rg = last_rg(b[4:], q0 + l - 4)
    f["end_key"] = (lib_of.get(rg, 0), r["tid"], end - 1 + trail if rev else r["pos"] - lead, rev)
    f["score"] = min(sum(q for q in b[q0:q0 + l] if q >= 15), SCORE_MAX)
    f["paired"] = bool(flag & 1) and not (flag & 8)
    return f


def compute(recs, rg=(), lib_of_rg=()):
    """recs: the stream as view_reference.records gives it; (the set of duplicate ordinals, the counts by name)"""
    lib_of = {}
    for g, lb in zip(rg, lib_of_rg):
        lib_of.setdefault(g if isinstance(g, bytes) else g.encode(), lb)
    fs = [facts(r, lib_of) for r in recs]
    dup = set()
    # the mate join, in ordinal order
    held, pairs = {}, []
    for o, f in enumerate(fs):
        if not f["taking"] or not f["paired"]:
            continue
        h = held.get(f["name"])
        if h is None:
            held[f["name"]] = o
        elif fs[h]["flag"] & 0xc0 == f["flag"] & 0xc0:
            pass
        else:
            pairs.append((h, o))
            del held[f["name"]]
    # pairs of one pair key: the highest score, then the smallest pair ordinal
    groups = {}
    for a, b in pairs:
        ka, kb = fs[a]["end_key"], fs[b]["end_key"]
        first, second = (ka, kb) if (ka[1:], ka[0]) <= (kb[1:], kb[0]) else (kb, ka)
        groups.setdefault((first, second), []).append((a, b))
    dup_paired = 0
    for members in groups.values():
        best = None
        for a, b in members:
            s = fs[a]["score"] + fs[b]["score"]
            if best is None or s > best[0] or (s == best[0] and min(a, b) < best[1]):
                best = (s, min(a, b))
        for a, b in members:
            if min(a, b) != best[1]:
                dup.update((a, b))
                dup_paired += 2
    # the taking-part records of one end key
    ends = {}
    for o, f in enumerate(fs):
        if f["taking"]:
            ends.setdefault(f["end_key"], []).append(o)
    dup_frags = 0
    for members in ends.values():
        frags = [o for o in members if not fs[o]["paired"]]
        keep = None
        if len(frags) == len(members):
            for o in frags:
                if keep is None or fs[o]["score"] > fs[keep]["score"]:
                    keep = o
        for o in frags:
            if o != keep:
                dup.add(o)
                dup_frags += 1
    n_paired = sum(1 for f in fs if f["taking"] and f["paired"])
    n_taking = sum(1 for f in fs if f["taking"])
    counts = {"records": len(fs), "taking_part": n_taking, "paired": n_paired, "pairs": len(pairs), "unmatched": n_paired - 2 * len(pairs),
              "fragments": n_taking - n_paired, "dup_paired": dup_paired, "dup_fragments": dup_frags}
    return dup, counts


def expected_bytes(recs, dup, remove=False):
    """the stream behind the command: the taking-part records with 0x400 from `dup' (or without the duplicates), the others as they came"""
    out = []
    for o, r in enumerate(recs):
        b = bytearray(r["bytes"])
        nc, = struct.unpack_from("<H", b, 16)
        if not (r["flag"] & 0x904) and nc > 0:
            if remove and o in dup:
                continue
            b[19] = (b[19] & ~4) | (4 if o in dup else 0)
        out.append(bytes(b))
    return out
