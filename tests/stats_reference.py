"""A model of ssg_stats_* and of what `sambamba stats' counts that shares no code with the product or its kernels: records are decoded with struct, the filter is
view_reference's (a translation of the expression to Python), every counter is an entry of a plain dict filled record by record and base by base from the
definitions of include/ssgpu.h, the checksums are zlib.crc32 over the byte ranges named there, and coverage is a model of intervals: the depth between two
neighbouring ends of reads is constant, so the histogram is a sum of stretch lengths."""
import struct
import zlib
from collections import defaultdict

import numpy as np

import view_reference as ref

NGC, NINDEL, M32, M64 = 200, 300, (1 << 32) - 1, (1 << 64) - 1
SCALARS = ("filtered", "secondary", "dup", "dup_len", "max_len", "total_len", "qcfail", "paired", "first", "last", "unmapped", "bases_mapped", "mq0", "single",
           "paired_mapped", "proper", "anomalous", "mismatches", "bases_cigar", "sum_qual", "max_qual", "chk_names", "chk_reads", "chk_quals", "sorted")
TABLES = ("quals", "bases", "gc", "isize", "rl", "id", "ic", "cov")
BASE_COLUMN = {1: 0, 2: 1, 4: 2, 8: 3, 15: 4}   # A C G T N; everything else, `=' among them: 5
AUX_SIZE = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
AUX_INT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<i"}   # bam_aux2i returns an int32_t: an I above 2^31 - 1 reads negative


def rounded_cov(cov_min, cov_max, cov_step):
    """(cov_max, cov_step, bins) as init_stat_structs rounds them"""
    if cov_step > cov_max - cov_min + 1:
        cov_step = cov_max - cov_min
        if cov_step <= 0:
            cov_step = 1
    n = 3 + (cov_max - cov_min) // cov_step
    return cov_min + ((cov_max - cov_min) // cov_step + 1) * cov_step - 1, cov_step, n


def first_nm(b, a):
    """the value of the first NM tag of the aux area b[a:], or None: an unknown type, a Z / H without NUL, a B or a value cut short end the walk"""
    e = len(b)
    while a + 3 <= e:
        tag, ty = b[a:a + 2], chr(b[a + 2])
        a += 3
        if ty in AUX_SIZE:
            sz = AUX_SIZE[ty]
        elif ty in "ZH":
            q = b.find(0, a)
            if q < 0:
                return None
            sz = q - a + 1
        elif ty == "B":
            if a + 5 > e:
                return None
            sz = 5 + {"c": 1, "C": 1, "s": 2, "S": 2}.get(chr(b[a]), 4) * struct.unpack_from("<I", b, a + 1)[0]
        else:
            return None
        if a + sz > e:
            return None
        if tag == b"NM":
            return struct.unpack_from(AUX_INT[ty], b, a)[0] if ty in AUX_INT else 0
        a += sz
    return None


def compute(recs, expr="", max_len=1024, n_isize=8000, cov_min=1, cov_max=1000, cov_step=1):
    """the scalars by name and the tables as uint64 arrays, shaped as capi.stats_get shapes them, of the records of view_reference.records"""
    sc = dict.fromkeys(SCALARS, 0)
    quals, bases, gc, isz, rl, ind, ic = (defaultdict(int) for _ in range(7))
    covered = []
    for r in recs:
        b, flag, l_seq = r["bytes"], r["flag"], r["l_seq"]
        if not ref.passes(expr, r):
            sc["filtered"] += 1
            continue
        l_qname, nc = b[12], struct.unpack_from("<H", b, 16)[0]
        name = b[36:36 + l_qname]
        name = name[:name.index(0)] if 0 in name else name
        s0 = 36 + l_qname + 4 * nc
        half = (l_seq + 1) // 2
        sc["chk_names"] = (sc["chk_names"] + zlib.crc32(name)) & M32
        if l_seq:
            sc["chk_reads"] = (sc["chk_reads"] + zlib.crc32(b[s0:s0 + half])) & M32
            sc["chk_quals"] = (sc["chk_quals"] + zlib.crc32(b[s0 + half:s0 + 2 * half])) & M32
        if flag & 0x100:
            sc["secondary"] += 1
            continue
        if not l_seq:
            continue
        if flag & 0x400:
            sc["dup"] += 1
            sc["dup_len"] += l_seq
        ops = [(v >> 4, v & 0xf) for v in struct.unpack_from("<%dI" % nc, b, 36 + l_qname)]
        unclipped = l_seq + sum(n for n, op in ops if op == 5)
        sc["max_len"] = max(sc["max_len"], unclipped)
        rev, mapped = bool(flag & 0x10), not flag & 4
        both = bool(flag & 1) and not flag & 4 and not flag & 8
        if not flag & 0x900:
            frag = 1 if flag & 0x80 else 0
            rl[unclipped] += 1
            sc["total_len"] += l_seq
            sc["qcfail"] += 1 if flag & 0x200 else 0
            sc["paired"] += flag & 1
            sc["last" if frag else "first"] += 1
            g = 0
            for i in range(l_seq):
                cycle = l_seq - 1 - i if rev else i
                code = b[s0 + i // 2] >> (0 if i & 1 else 4) & 15
                bases[cycle, BASE_COLUMN.get(code, 5)] += 1
                g += code in (2, 4)
            for cycle in range(l_seq):
                q = b[s0 + half + (l_seq - 1 - cycle if rev else cycle)]
                quals[frag, cycle, q] += 1
                sc["sum_qual"] += q
                sc["max_qual"] = max(sc["max_qual"], q)
            for k in range(g * (NGC - 1) // l_seq, min((g + 1) * (NGC - 1) // l_seq, NGC - 1)):
                gc[frag, k] += 1
            if not mapped:
                sc["unmapped"] += 1
            else:
                sc["bases_mapped"] += l_seq
                sc["mq0"] += r["mapq"] == 0
                sc["paired_mapped" if both else "single"] += 1
                if both:
                    sc["proper"] += 1 if flag & 2 else 0
                    sc["anomalous"] += r["tid"] != r["mtid"]
        if not mapped:
            continue
        f1, cyc = 0 if flag & 0x40 else 1, 0
        for n, op in ops:
            if n == 0:
                continue
            if op == 1:
                ic[f1, l_seq - cyc - n if rev else cyc] += 1
                cyc += n
                if n <= NINDEL:
                    ind[0, n - 1] += 1
            elif op == 2:
                at = l_seq - cyc - 1 if rev else cyc - 1
                if at >= 0:
                    ic[2 + f1, at] += 1
                    if n <= NINDEL:
                        ind[1, n - 1] += 1
            elif op not in (3, 5, 6):
                cyc += n
        if both:
            a = min(abs(r["isize"]), n_isize - 1)
            if a > 0 or r["tid"] == r["mtid"]:
                d = r["mpos"] - r["pos"]
                sf, sw, sm = (1 if flag & 0x40 else -1), (-1 if rev else 1), (-1 if flag & 0x20 else 1)
                if sw * sm > 0:
                    isz[2, a] += 1
                elif sf * d > 0:
                    isz[0 if sf * sw > 0 else 1, a] += 1
                elif sf * d < 0:
                    isz[1 if sf * sw > 0 else 0, a] += 1
        nm = first_nm(b, s0 + half + l_seq)
        sc["mismatches"] = (sc["mismatches"] + (nm or 0)) & M64
        sc["bases_cigar"] += sum(n for n, op in ops if op in (0, 1))
        covered.append((r["tid"] & M32, r["pos"] & M32, l_seq))
    # coverage: only of a stream whose covered records never descend
    cov_max, cov_step, n_cov = rounded_cov(cov_min, cov_max, cov_step)
    cov = [0] * n_cov
    sc["sorted"] = 1 if all(covered[k][:2] <= covered[k + 1][:2] for k in range(len(covered) - 1)) else 0
    if sc["sorted"]:
        ends = defaultdict(lambda: defaultdict(int))
        for tid, pos, n in covered:
            ends[tid][pos] += 1
            ends[tid][pos + n] -= 1
        for ev in ends.values():
            depth, at = 0, None
            for p in sorted(ev):
                if depth:
                    cov[0 if depth < cov_min else n_cov - 1 if depth > cov_max else 1 + (depth - cov_min) // cov_step] += p - at
                depth, at = depth + ev[p], p
    rows = max_len + 1
    shapes = {"quals": (2, rows, 256), "bases": (rows, 6), "gc": (2, NGC), "isize": (3, n_isize), "rl": (rows,), "id": (2, NINDEL), "ic": (4, rows)}
    out = dict(sc)
    for name, d in (("quals", quals), ("bases", bases), ("gc", gc), ("isize", isz), ("rl", rl), ("id", ind), ("ic", ic)):
        a = np.zeros(shapes[name], dtype=np.uint64)
        for k, v in d.items():
            a[k] = v // 2 if name == "isize" else v
        out[name] = a
    out["cov"] = np.array(cov, dtype=np.uint64)
    return out


def differences(got, want):
    """the names of the scalars and tables in which two results differ"""
    return [k for k in SCALARS if int(got[k]) != int(want[k])] + [k for k in TABLES if got[k].shape != want[k].shape or not (got[k] == want[k]).all()]
