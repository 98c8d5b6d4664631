"""Independent reference of the seeding stage (mem_collect_intv's interval list; the seeds mem_chain visits: bwt_sa + bns_intv2rid + the max_occ
sub-sampling) -- TEST INFRASTRUCTURE ONLY.

Seeding has a definition in terms of the text alone: how often does this substring of the read occur in T2 = fwd || revcomp(fwd), and where.  This
module is that definition.  It imports neither oracle_py nor speedseq_amd.capi, and shares nothing with oracle/orc_mem.c, oracle/orc_index.c or the
kernels.

What it is independent in -- algorithm as well as hand:
  * the suffix array of T2 is made by SORTING (prefix doubling over numpy keys): no BWT, no occurrence tables, no bidirectional intervals, no LF
    walk over sampled rows.  A shorter suffix sorts before its extensions (what upstream's sentinel does).
  * rank(P) and occ(P) are binary searches over that array with Python's own bytes comparison of text slices (`T2[sa:sa + len(P)]`): a shorter
    slice sorts before its extensions there too.  No interval is ever extended by a base; every (s, e) a pass asks for is looked up whole.
  * the three passes are written from their definitions (the supermaximal matches of the read; the matches around a point that keep m occurrences;
    the first prefix rarer than max_mem_intv), not from upstream's visiting order: no forward sweep that records where the count changes, no
    backward sweep over the recorded list.
  * the forward bases come from .pac + .ann (the index's own 2-bit text, ambiguous bases already replaced), the contig table from .ann.
A twin that shares nothing with the suffix array checks rank, occ and SA on tiny texts (`*_plain`: sliding-window comparison, sorted() over Python
strings), as `*_scalar` does in dp_reference.py.

Definitions.  n = len(T2); SA = the suffix array; for a pattern P of codes 0..3
    rank(P) = number of suffixes of T2 smaller than P          occ(P) = number of suffixes that start with P
and a substring of the read with an N in it (code > 3) occurs nowhere.  The interval of read substring q[s:e]:
    x0 = rank(q[s:e]) + 1        x1 = rank(revcomp(q[s:e])) + 1        x2 = occ(q[s:e])        info = s << 32 | e
(the + 1 is the row of the sentinel: row r >= 1 of upstream's BWT matrix is SA[r - 1]; row 0 is the empty suffix).
The list of mem_collect_intv is pass 1 + pass 2 + pass 3, sorted by info (equal info means equal fields, so an unstable sort cannot show):
  pass 1  every (s, e) that occurs and cannot be extended on either side and still occur, of length >= min_seed_len: with L[s] the longest matching
          end from s, (s, L[s]) where L[s] > s and L[s - 1] < L[s].
  pass 2  for every pass-1 match, in pass-1 order, with e - s >= (int)(min_seed_len * split_factor + .499) and x2 <= split_width: x = (s + e) >> 1,
          m = x2 + 1; every (s', e') with s' <= x < e' that occurs >= m times and cannot be extended on either side and still occur >= m times,
          of length >= min_seed_len.
  pass 3  only when max_mem_intv > 0.  From x = 0: at an N, step one base; else the smallest i > x with q[i] not N, i - x >= min_seed_len and
          occ(q[x:i + 1]) < max_mem_intv -- (x, i + 1) is kept when it occurs at all, and the pass continues at i + 1; an N met first continues
          after it; running out of read ends the pass.
The seeds, for each interval in list order: step = x2 / max_occ when x2 > max_occ, else 1; k = 0, step, 2 * step, ... while k < x2 and fewer than
max_occ were taken: rbeg = SA[x0 - 1 + k], qbeg = s, len = e - s.  rid: a seed with rbeg >= l_pac is mapped to the forward strand (its first base
to 2 * l_pac - 1 - rbeg); rid is the contig that holds the seed's first and last base, -1 when they lie in different contigs, and -2 when the
seed spans the junction of the two strands (upstream's bns_intv2rid tells the two apart by that value; mem_chain drops both).

Cost, measured 2026-10-17 on a CPU-only build host (x86-64, one core): the suffix array of the golden slice (643 270 doubled bases) takes 0.4 s, once per
text; the interval list and the seeds of a read take 2 to 5 ms (150 bases; the first prototype of these definitions, which walked 160 000-row slices in
numpy, took 1.4 s).  The not-gpu part of tests/test_seed_reference.py takes 10 s in all, the oracle's and the emulator's runs included.
"""
import bisect
import collections

import numpy as np

SeedOpts = collections.namedtuple("SeedOpts", "min_seed_len split_factor split_width max_occ max_mem_intv")
DEFAULTS = SeedOpts(19, 1.5, 10, 500, 20)


def suffix_array(t2):
    """suffix array of codes 0..3 by prefix doubling: keys of the first 12 bases (digits 1..4, 0 beyond the end, so a shorter suffix sorts first),
    then rank pairs (rank[i], rank[i + k]) until every rank is its own"""
    t2 = np.asarray(t2, dtype=np.int64)
    n = t2.size
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    k = 12
    pad = np.concatenate([t2 + 1, np.zeros(k, dtype=np.int64)])
    key = np.zeros(n, dtype=np.int64)
    for j in range(k):
        key = key * 5 + pad[j:j + n]
    while True:
        _, rank = np.unique(key, return_inverse=True)
        rank = rank.astype(np.int64).reshape(-1)
        if int(rank.max()) == n - 1 or k >= n:
            break
        nxt = np.zeros(n, dtype=np.int64)
        nxt[:n - k] = rank[k:] + 1
        key = rank * (n + 1) + nxt
        k *= 2
    sa = np.empty(n, dtype=np.int64)
    sa[rank] = np.arange(n, dtype=np.int64)
    return sa


# ---------------------------------------------------------------- the twin: nothing shared with the suffix array
def suffix_array_plain(t2):
    s = "".join("ACGT"[c] for c in t2)
    return sorted(range(len(s)), key=lambda i: s[i:])


def occ_plain(t2, p):
    t, p = [int(c) for c in t2], [int(c) for c in p]
    if any(c > 3 for c in p):
        return 0
    return sum(1 for i in range(len(t) - len(p) + 1) if t[i:i + len(p)] == p)


def rank_plain(t2, p):
    s, ps = "".join("ACGT"[c] for c in t2), "".join("ACGT"[c] for c in p)
    return sum(1 for i in range(len(s)) if s[i:] < ps)


def revcomp(p):
    return [3 - int(c) for c in reversed(p)]


class SeedRef:
    """the doubled text of an index and its suffix array; collect_intv() and seeds() of a read"""

    def __init__(self, fwd, ctg_off=None, ctg_len=None):
        fwd = np.asarray(fwd, dtype=np.uint8)
        assert fwd.size == 0 or int(fwd.max()) <= 3
        self.l_pac = int(fwd.size)
        self.t2 = np.concatenate([fwd, (3 - fwd[::-1]).astype(np.uint8)])
        self.n = int(self.t2.size)
        self.ctg_off = [0] if ctg_off is None else [int(x) for x in ctg_off]
        self.ctg_len = [self.l_pac] if ctg_len is None else [int(x) for x in ctg_len]
        self.sa_np = suffix_array(self.t2)
        self.sa = self.sa_np.tolist()
        self._tb = self.t2.tobytes()

    @classmethod
    def from_index(cls, prefix):
        """forward bases from prefix.pac (four bases a byte, the first in the top bits), lengths and offsets from prefix.ann"""
        ann = open(prefix + ".ann").read().split("\n")
        l_pac, n_seq = int(ann[0].split()[0]), int(ann[0].split()[1])
        pac = np.fromfile(prefix + ".pac", dtype=np.uint8)
        codes = np.empty(pac.size * 4, dtype=np.uint8)
        for k in range(4):
            codes[k::4] = (pac >> (6 - 2 * k)) & 3
        off = [int(ann[2 + 2 * i].split()[0]) for i in range(n_seq)]
        ln = [int(ann[2 + 2 * i].split()[1]) for i in range(n_seq)]
        assert sum(ln) == l_pac and off == [sum(ln[:i]) for i in range(n_seq)]
        return cls(codes[:l_pac], off, ln)

    # ---- rank / occ
    def _range(self, p):
        """[lo, hi): the suffixes that start with p (bytes of codes 0..3)"""
        tb, m = self._tb, len(p)
        key = lambda i: tb[i:i + m]
        lo = bisect.bisect_left(self.sa, p, key=key)
        return lo, bisect.bisect_right(self.sa, p, lo=lo, key=key)

    def rank(self, p):
        return self._range(bytes(bytearray(int(c) for c in p)))[0]

    def occ(self, p):
        if any(int(c) > 3 for c in p):
            return 0
        lo, hi = self._range(bytes(bytearray(int(c) for c in p)))
        return hi - lo

    def _occ_b(self, qb, s, e):
        """occ of read substring qb[s:e] (bytes; the caller keeps N out)"""
        lo, hi = self._range(qb[s:e])
        return hi - lo

    def interval(self, q, s, e):
        p = [int(c) for c in q[s:e]]
        lo, hi = self._range(bytes(bytearray(p)))
        return (lo + 1, self.rank(revcomp(p)) + 1, hi - lo, s << 32 | e)

    # ---- the passes
    @staticmethod
    def _longest(n, has_n, at_least):
        """L[s] for every s: the largest e with at_least(s, e) true (e = s where not even one base is), for a predicate that is monotone
        (true for (s, e) -> true for (s + 1, e) and (s, e - 1)): so L[s + 1] >= L[s] - 1 and the end never moves back"""
        L, e = [0] * n, 0
        for s in range(n):
            if has_n[s]:
                L[s] = s
                e = s + 1
                continue
            e = max(e, s)
            while e < n and not has_n[e] and at_least(s, e + 1):
                e += 1
            L[s] = e
        return L

    def collect_intv(self, q, opt=DEFAULTS, passes=False):
        """the interval list of a read as (x0, x1, x2, info) tuples, sorted by info; passes=True: also the number of intervals each pass kept"""
        q = [int(c) for c in q]
        n = len(q)
        has_n = [c > 3 for c in q]
        qb = bytes(bytearray(min(c, 4) for c in q))
        msl = int(opt.min_seed_len)
        out = []
        # pass 1
        L = self._longest(n, has_n, lambda s, e: self._occ_b(qb, s, e) >= 1)
        p1 = [(s, L[s]) for s in range(n) if L[s] > s and (s == 0 or L[s - 1] < L[s])]
        p1 = [self.interval(q, s, e) for s, e in p1 if e - s >= msl]
        out += p1
        # pass 2
        split_len = int(float(np.float32(msl) * np.float32(opt.split_factor)) + .499)
        n2 = 0
        for x0, x1, x2, info in p1:
            s, e = info >> 32, info & 0xffffffff
            if e - s < split_len or x2 > opt.split_width:
                continue
            x, m = (s + e) >> 1, x2 + 1
            lo = x                                   # the leftmost start from which a match through x still occurs m times
            if self._occ_b(qb, x, x + 1) < m:
                continue
            while lo > 0 and not has_n[lo - 1] and self._occ_b(qb, lo - 1, x + 1) >= m:
                lo -= 1
            prev_end, e2 = -1, x + 1
            for s2 in range(lo, x + 1):
                while e2 < n and not has_n[e2] and self._occ_b(qb, s2, e2 + 1) >= m:
                    e2 += 1
                if e2 > prev_end:                    # not extendable to the left: one base more on the left ended earlier (or did not reach x)
                    if e2 - s2 >= msl:
                        out.append(self.interval(q, s2, e2))
                        n2 += 1
                    prev_end = e2
        # pass 3
        n3 = 0
        if opt.max_mem_intv > 0:
            x = 0
            while x < n:
                if has_n[x]:
                    x += 1
                    continue
                i = x + 1
                nxt = n
                while i < n:
                    if has_n[i]:
                        nxt = i + 1
                        break
                    if i - x >= msl:
                        c = self._occ_b(qb, x, i + 1)
                        if c < opt.max_mem_intv:
                            if c > 0:
                                out.append(self.interval(q, x, i + 1))
                                n3 += 1
                            nxt = i + 1
                            break
                    i += 1
                x = nxt
        out.sort(key=lambda t: t[3])
        return (out, (len(p1), n2, n3)) if passes else out

    # ---- seeds
    def rid(self, rbeg, ln):
        if rbeg < self.l_pac < rbeg + ln:
            return -2
        first, last = rbeg, rbeg + ln - 1
        if rbeg >= self.l_pac:
            first, last = 2 * self.l_pac - 1 - first, 2 * self.l_pac - 1 - last
        holds = lambda p: [k for k in range(len(self.ctg_off)) if self.ctg_off[k] <= p < self.ctg_off[k] + self.ctg_len[k]]
        a, b = holds(first), holds(last)
        assert len(a) == 1 and len(b) == 1
        return a[0] if a == b else -1

    def seeds_of(self, intvs, opt=DEFAULTS):
        out = []
        for x0, x1, x2, info in intvs:
            s, e = info >> 32, info & 0xffffffff
            step = x2 // opt.max_occ if x2 > opt.max_occ else 1
            k = taken = 0
            while k < x2 and taken < opt.max_occ:
                rbeg = self.sa[x0 - 1 + k]
                out.append((rbeg, s, e - s, self.rid(rbeg, e - s)))
                k += step
                taken += 1
        return out

    def seeds(self, q, opt=DEFAULTS):
        return self.seeds_of(self.collect_intv(q, opt), opt)
