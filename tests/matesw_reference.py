"""Plain restatement of upstream mem_matesw and of mem_sort_dedup_patch as mem_matesw calls it (no patching) -- TEST
INFRASTRUCTURE ONLY.

Written from upstream's documented behaviour (bwamem_pair.c mem_matesw, bwamem.c mem_sort_dedup_patch), not from csrc/k_pair.h, csrc/k_sdp.h or
csrc/k_mswkeys.h.  It imports neither oracle_py nor speedseq_amd.capi: the alignment of a window is a function the caller hands in (the oracle's
orc_api_align2 in the tests: ksw_align2's result (score, te, qe, score2, te2, tb, qb) for a query, a target and the xtra word).

Lists are Python lists of dicts with the fields of mem_alnreg_t (the library's ALNREG_DT names).  Both sorts of mem_sort_dedup_patch are unstable
in upstream (ks_introsort): what they do with equal keys is not a property of the inputs, so `sort_dedup' RAISES Tie when two regions share `re'
or share (score, rb, qb).  A test whose inputs are meant to be decided by values alone must pass without that exception.

Arithmetic: integers; the one real comparison, overlap > mask_level_redun * length, is a float32 product compared in float32 as in C (the lengths
are far below 2^24, so the conversions are exact and only the product rounds).
"""
import numpy as np

KSW_XBYTE, KSW_XSTOP, KSW_XSUBO, KSW_XSTART = 0x10000, 0x20000, 0x40000, 0x80000
FIELDS = ("rb", "re", "qb", "qe", "rid", "score", "truesc", "sub", "alt_sc", "csub", "sub_n", "w", "seedcov", "secondary", "secondary_all", "seedlen0", "n_comp",
          "frac_rep", "hash")
DEFAULTS = dict(a=1, min_seed_len=19, pen_unpaired=17, max_matesw=50, max_chain_gap=10000, mask_level_redun=0.95)


class Tie(Exception):
    """the outcome would depend on what an unstable sort does with equal keys"""


def opt_from(rec=None, **kw):
    o = dict(DEFAULTS)
    if rec is not None:
        for k in DEFAULTS:
            o[k] = rec[k].item() if hasattr(rec[k], "item") else rec[k]
    o.update(kw)
    o["mask_level_redun"] = np.float32(o["mask_level_redun"])
    return o


def regs_from(arr):
    out = []
    for a in arr:
        d = {f: (float(a[f]) if f == "frac_rep" else int(a[f])) for f in FIELDS}
        out.append(d)
    return out


class Ref:
    """the doubled reference of an index: forward bases from prefix.pac, contigs from prefix.ann; position p >= l_pac is the complement of 2 l_pac - 1 - p"""

    def __init__(self, prefix):
        ann = open(prefix + ".ann").read().split("\n")
        self.l_pac, n_seq = int(ann[0].split()[0]), int(ann[0].split()[1])
        pac = np.fromfile(prefix + ".pac", dtype=np.uint8)
        codes = np.empty(pac.size * 4, dtype=np.uint8)
        for k in range(4):
            codes[k::4] = (pac >> (6 - 2 * k)) & 3
        fwd = codes[:self.l_pac]
        self.t2 = np.concatenate([fwd, (3 - fwd[::-1]).astype(np.uint8)])
        self.ctg_off = [int(ann[2 + 2 * i].split()[0]) for i in range(n_seq)]
        self.ctg_len = [int(ann[2 + 2 * i].split()[1]) for i in range(n_seq)]

    def rid_of(self, pos):
        """contig of a doubled coordinate"""
        f = pos if pos < self.l_pac else 2 * self.l_pac - 1 - pos
        for i in range(len(self.ctg_off)):
            if self.ctg_off[i] <= f < self.ctg_off[i] + self.ctg_len[i]:
                return i
        return -1

    def fetch(self, rb, mid, re):
        """upstream bns_fetch_seq: [rb, re) cut to the contig (and strand) that holds mid; (rb, re, rid)"""
        rid = self.rid_of(mid)
        beg, end = self.ctg_off[rid], self.ctg_off[rid] + self.ctg_len[rid]
        if mid >= self.l_pac:
            beg, end = 2 * self.l_pac - end, 2 * self.l_pac - beg
        return max(rb, beg), min(re, end), rid


def infer_dir(l_pac, b1, b2):
    r1, r2 = b1 >= l_pac, b2 >= l_pac
    p2 = b2 if r1 == r2 else 2 * l_pac - 1 - b2
    return (0 if r1 == r2 else 1) ^ (0 if p2 > b1 else 3), abs(p2 - b1)


def _redundant(opt, p, q):
    """p ends after q: do they cover one another on the reference and on the query beyond mask_level_redun of the shorter?"""
    m = opt["mask_level_redun"]
    or_ = q["re"] - p["rb"]
    oq = q["qe"] - p["qb"] if q["qb"] < p["qb"] else p["qe"] - q["qb"]
    mr = min(q["re"] - q["rb"], p["re"] - p["rb"])
    mq = min(q["qe"] - q["qb"], p["qe"] - p["qb"])
    return bool(np.float32(or_) > m * np.float32(mr)) and bool(np.float32(oq) > m * np.float32(mq))


def sort_dedup(opt, regs):
    """mem_sort_dedup_patch without patching; a new list of copies"""
    a = [dict(r) for r in regs]
    if len(a) <= 1:
        return a
    if len({r["re"] for r in a}) != len(a):
        raise Tie("two regions end at the same reference position")
    a.sort(key=lambda r: r["re"])
    for r in a:
        r["n_comp"] = 1
    gap = opt["max_chain_gap"]
    for i in range(1, len(a)):
        p = a[i]
        if p["rid"] != a[i - 1]["rid"] or p["rb"] >= a[i - 1]["re"] + gap:
            continue
        j = i - 1
        while j >= 0 and p["rid"] == a[j]["rid"] and p["rb"] < a[j]["re"] + gap:
            q = a[j]
            j -= 1
            if q["qe"] == q["qb"]:
                continue
            if _redundant(opt, p, q):
                if p["score"] < q["score"]:
                    p["qe"] = p["qb"]
                    break
                q["qe"] = q["qb"]
    a = [r for r in a if r["qe"] > r["qb"]]
    if len({(r["score"], r["rb"], r["qb"]) for r in a}) != len(a):
        raise Tie("two regions share (score, rb, qb)")
    a.sort(key=lambda r: (-r["score"], r["rb"], r["qb"]))
    return a


def new_region():
    d = {f: 0 for f in FIELDS}
    d["frac_rep"] = 0.0
    return d


def matesw(opt, ref, pes, anchor, ms, ma, align2, tally):
    """mem_matesw for one anchor against the mate's list ma (replaced, not modified); ms: the mate's bases; pes: four dicts (low, high, failed).
    Returns (windows tried, the new list).  tally: dict with 'windows' and 'cells'."""
    l_pac, l_ms = ref.l_pac, len(ms)
    skip = [1 if pes[r]["failed"] else 0 for r in range(4)]
    for y in ma:
        r, dist = infer_dir(l_pac, anchor["rb"], y["rb"])
        if pes[r]["low"] <= dist <= pes[r]["high"]:
            skip[r] = 1
    if sum(skip) == 4:
        return 0, ma
    n, rid = 0, -1
    for r in range(4):
        if skip[r]:
            continue
        is_rev, is_larger = (r >> 1) != (r & 1), not (r >> 1)
        seq = (3 - ms[::-1]).astype(np.uint8) if is_rev else ms
        seq = np.where((ms[::-1] if is_rev else ms) > 3, 4, seq).astype(np.uint8)
        lo, hi = pes[r]["low"], pes[r]["high"]
        if not is_rev:
            rb = anchor["rb"] + lo if is_larger else anchor["rb"] - hi
            re = (anchor["rb"] + hi if is_larger else anchor["rb"] - lo) + l_ms
        else:
            rb = (anchor["rb"] + lo if is_larger else anchor["rb"] - hi) - l_ms
            re = anchor["rb"] + hi if is_larger else anchor["rb"] - lo
        rb, re = max(rb, 0), min(re, 2 * l_pac)
        if rb < re:
            rb, re, rid = ref.fetch(rb, (rb + re) >> 1, re)
        if anchor["rid"] == rid and re - rb >= opt["min_seed_len"]:
            xtra = KSW_XSUBO | KSW_XSTART | (KSW_XBYTE if l_ms * opt["a"] < 250 else 0) | (opt["min_seed_len"] * opt["a"])
            score, te, qe, score2, te2, tb, qb = align2(np.ascontiguousarray(seq), np.ascontiguousarray(ref.t2[rb:re]), xtra)
            tally["windows"] += 1
            tally["cells"] += (re - rb) * l_ms
            if score >= opt["min_seed_len"] and qb >= 0:
                b = new_region()
                b["rid"] = anchor["rid"]
                b["qb"] = l_ms - (qe + 1) if is_rev else qb
                b["qe"] = l_ms - qb if is_rev else qe + 1
                b["rb"] = 2 * l_pac - (rb + te + 1) if is_rev else rb + tb
                b["re"] = 2 * l_pac - (rb + tb) if is_rev else rb + te + 1
                b["score"], b["csub"], b["secondary"] = score, score2, -1
                b["seedcov"] = min(b["re"] - b["rb"], b["qe"] - b["qb"]) >> 1
                at = next((i for i, y in enumerate(ma) if y["score"] < b["score"]), len(ma))
                ma = ma[:at] + [b] + ma[at:]
            n += 1
        if n:
            ma = sort_dedup(opt, ma)
    return n, ma


def rescue_pair(opt, ref, pes, reads, lists, align2):
    """mem_sam_pe's rescue loop for one pair: reads = (bases of read 1, of read 2), lists = (regions of read 1, of read 2).
    Returns (the two lists after rescue, tally)."""
    a = [[dict(r) for r in lists[0]], [dict(r) for r in lists[1]]]
    tally = dict(windows=0, cells=0)
    b = [[], []]
    for i in range(2):
        for r in a[i]:
            if r["score"] >= a[i][0]["score"] - opt["pen_unpaired"]:
                b[i].append(dict(r))
        b[i] = b[i][:opt["max_matesw"]]
    for i in range(2):
        for anchor in b[i]:
            _, a[1 - i] = matesw(opt, ref, pes, anchor, reads[1 - i], a[1 - i], align2, tally)
    return a, tally
