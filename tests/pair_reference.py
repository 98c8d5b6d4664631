"""Independent reference of the paired-end decision stage (mem_pestat, mem_mark_primary_se, mem_pair, mem_approx_mapq_se, the decision tree of
mem_sam_pe and the record list of mem_reg2sam with its XA candidates) -- TEST INFRASTRUCTURE ONLY.

Written from SURVEY.md Appendix B and from upstream's documented behaviour (bwamem.c, bwamem_pair.c), not from csrc/k_pair.h, csrc/k_pairw.h or
oracle/orc_pair.c.  It imports neither oracle_py nor speedseq_amd.capi.  What it shares with them, and only this:
  * the constants (0.499, 6.02, 4.343, 0.721, the quartile fractions, the 2 / 3 IQR fences, 4 std, 0.8, 10, 0.05, the option block's values);
  * the integer hash hash_64 (Thomas Wang's 64-bit mix) and what is fed to it -- input index + id for a region, the two ranks in the position-sorted
    list of both ends for a candidate pair.  The hash is data (it only breaks ties), not an algorithm under test.

Arithmetic.  Integers and fractions.Fraction for everything rational; double and float constants enter at their binary values (Fraction(0.499),
Fraction(numpy.float32(mask_level)), frac_rep as the float32 it is stored as, avg and std of an insert-size model as the doubles they are stored as,
M_SQRT1_2 as the double it is); the sum frac_rep[0] + frac_rep[1] of mem_sam_pe is a float32 sum in C and is taken as one.  log, erfc and sqrt come
from mpmath at 60 digits; where a float64 first pass leaves the truncation more than 1e-6 (relative to max(1, |x|)) from an integer, its answer
stands and mpmath is not asked.

Truncation sites.  Every (int)(x + .499) goes through Sites.trunc, every comparison of an integer with a real that is not rational through
Sites.compare.  A site's margin is the distance of the exact real x + .499 from the nearest integer (of the two sides of the comparison); a site is
NEAR when margin < 1e-9 * max(1, |x|).  Where that threshold comes from: |x| < 2^11 on this path, a value goes through at most 12 roundings, and a
rounding is at most 16 ulp if the libm is that good: 12 * 16 * 2^-53 * 2^11 = 4.4e-11 absolute; 1e-9 is more than 20 times that.  The 16 ulp for
the device's log and erfc are an ASSUMPTION: nobody has measured the device's libm on this path beyond profiles/r05_libm_probe.txt.
A near site may legitimately fall to either side in binary64; `alternatives' re-evaluates a function with every subset of its near sites flipped to
the other neighbour, and a result under test may equal any of those.  Everything else must be equal.

Where 2 * erfc(...) underflows to zero in binary64 upstream's cast of log(0) is undefined: `pair' raises there (|ns| beyond about 38).

What is a second restatement rather than a definition: mem_mark_primary_se's greedy scan (a region is secondary to the FIRST earlier primary it
overlaps, and what `sub' and `sub_n' become depends on that order) has no definition as a set, so `mark_primary' is the loop again, in another
hand -- as dp_reference.py says of the extension.  `pair', `pestat' and `mapq_se' are definitions: no loop over a sorted array that stops early,
no capacity, no histogram.
"""
import math
from fractions import Fraction as F

import mpmath
import numpy as np

MP = mpmath.mp.clone()
MP.dps = 60

C499 = F(0.499)
NEAR_REL = 1e-9
FAST_REL = 1e-6

DEFAULTS = dict(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, pen_unpaired=17, T=30, min_seed_len=19, max_ins=10000, max_XA_hits=5, max_XA_hits_alt=200,
                mapQ_coef_fac=3, mapQ_coef_len=50.0, mask_level=0.5, XA_drop_ratio=0.8, flag=0)
F_NOPAIRING, F_NO_MULTI = 0x4, 0x10
MAIN, XA = 0, 1


def opt_from(rec=None, **kw):
    """the option values this stage reads, from a record with those field names (the library's option block) or the defaults, then kw"""
    o = dict(DEFAULTS)
    if rec is not None:
        for k in DEFAULTS:
            o[k] = rec[k].item() if hasattr(rec[k], "item") else rec[k]
    o.update(kw)
    for k in ("mapQ_coef_len", "mask_level", "XA_drop_ratio"):   # floats of the option block: their float32 values
        o[k] = float(np.float32(o[k]))
    return o


def hash_64(key):
    """Thomas Wang's 64-bit integer hash, as upstream's utils.h has it (shared data: see the header)"""
    m = (1 << 64) - 1
    key &= m
    key = (key + (~(key << 32) & m)) & m
    key ^= key >> 22
    key = (key + (~(key << 13) & m)) & m
    key ^= key >> 8
    key = (key + (key << 3)) & m
    key ^= key >> 15
    key = (key + (~(key << 27) & m)) & m
    key ^= key >> 31
    return key


class Sites:
    """the truncation and comparison sites of one evaluation: how many, which were near, the smallest relative margin; flips: ordinals of near sites
    that take the other neighbour in this evaluation"""

    def __init__(self, flips=()):
        self.n = 0
        self.near = []
        self.min_margin = math.inf
        self.flips = frozenset(flips)

    def _note(self, margin, scale):
        k = self.n
        self.n += 1
        rel = margin / max(1.0, scale)
        self.min_margin = min(self.min_margin, rel)
        is_near = rel < NEAR_REL
        if is_near:
            self.near.append(k)
        return is_near and k in self.flips

    def trunc(self, x, fast=None):
        """(int)(x + .499) of the exact real x (Fraction or mpf, or a callable giving the mpf); fast: the same value as a float64 first pass"""
        if fast is not None:
            y = fast + 0.499
            d = abs(y - round(y))
            if d > FAST_REL * max(1.0, abs(fast)):
                self._note(d, abs(fast))
                return int(y)
        if callable(x):
            x = x()
        if isinstance(x, F) or isinstance(x, int):
            y = F(x) + C499
            r = round(y)
            d, v, scale = abs(y - r), int(y), abs(float(x))
            other = int(2 * r - y)
            d = float(d)
        else:
            y = x + MP.mpf(C499.numerator) / C499.denominator
            r = MP.nint(y)
            d, scale = float(abs(y - r)), abs(float(x))
            v = int(MP.floor(y)) if y >= 0 else int(MP.ceil(y))
            yo = 2 * r - y
            other = int(MP.floor(yo)) if yo >= 0 else int(MP.ceil(yo))
        return other if self._note(d, scale) else v

    def compare_gt(self, x, y):
        """x > y where one side is an integer and the other a real (mpf, or a Fraction that binary64 cannot hold)"""
        d = abs(float(x - y))
        res = bool(x > y)
        return (not res) if self._note(d, abs(float(y))) else res

    def add(self, other):
        off = self.n
        self.n += other.n
        self.near += [off + k for k in other.near]
        self.min_margin = min(self.min_margin, other.min_margin)


def alternatives(fn, tally=None, max_near=6):
    """every result fn(sites) can have when its near sites may fall to either side: [exact result, results with near sites flipped ...]; tally: a Sites that
    receives the counts of the exact evaluation"""
    s = Sites()
    out = [fn(s)]
    if tally is not None:
        tally.add(s)
    if s.near:
        assert len(s.near) <= max_near, "too many near sites in one evaluation: choose other inputs"
        seen = {frozenset()}
        work = [frozenset([k]) for k in s.near]
        while work:                                   # a flip can bring other sites into play: follow them
            fl = work.pop()
            if fl in seen or len(fl) > max_near:
                continue
            seen.add(fl)
            s2 = Sites(fl)
            out.append(fn(s2))
            work += [fl | {k} for k in s2.near if k not in fl]
    return out


class Reg:
    """a region (upstream mem_alnreg_t), the fields this stage reads or writes; idx0: its index in the list as it was given"""
    __slots__ = ("rb", "re", "qb", "qe", "rid", "score", "sub", "csub", "sub_n", "seedcov", "frac_rep", "secondary", "secondary_all", "hash", "idx0")

    def __init__(self, rb, re, qb, qe, rid, score, csub=0, sub_n=0, seedcov=0, frac_rep=0.0, sub=0, idx0=-1):
        self.rb, self.re, self.qb, self.qe, self.rid, self.score = int(rb), int(re), int(qb), int(qe), int(rid), int(score)
        self.csub, self.sub_n, self.seedcov, self.sub = int(csub), int(sub_n), int(seedcov), int(sub)
        self.frac_rep = float(np.float32(frac_rep))
        self.secondary = self.secondary_all = -1
        self.hash = 0
        self.idx0 = idx0

    def copy(self):
        r = Reg(self.rb, self.re, self.qb, self.qe, self.rid, self.score, self.csub, self.sub_n, self.seedcov, self.frac_rep, self.sub, self.idx0)
        r.secondary, r.secondary_all, r.hash = self.secondary, self.secondary_all, self.hash
        return r


def regs_from(arr):
    """Reg list of the rows of a structured array with the library's field names"""
    return [Reg(a["rb"], a["re"], a["qb"], a["qe"], a["rid"], a["score"], a["csub"], a["sub_n"], a["seedcov"], a["frac_rep"], a["sub"], i) for i, a in enumerate(arr)]


class Pes:
    """an orientation's insert-size model; avg and std exact (Fraction or mpf) or the doubles they are stored as"""
    __slots__ = ("low", "high", "failed", "avg", "std", "n")

    def __init__(self, low=0, high=0, failed=1, avg=0, std=0, n=0):
        self.low, self.high, self.failed, self.avg, self.std, self.n = low, high, failed, avg, std, n      # n: insert sizes that went into avg and std


def _max_pen(opt):
    return max(opt["a"] + opt["b"], opt["o_del"] + opt["e_del"], opt["o_ins"] + opt["e_ins"])


def _overlaps(x, y, mask_level):
    """the two query intervals overlap by at least mask_level of the shorter one"""
    b_max, e_min = max(x.qb, y.qb), min(x.qe, y.qe)
    return e_min > b_max and e_min - b_max >= min(x.qe - x.qb, y.qe - y.qb) * F(mask_level)


def infer_dir(l_pac, b1, b2):
    """(orientation 0..3 = FF, FR, RF, RR; distance) of two doubled-strand coordinates: the second is brought to the first one's strand"""
    r1, r2 = b1 >= l_pac, b2 >= l_pac
    p2 = b2 if r1 == r2 else 2 * l_pac - 1 - b2
    return (0 if r1 == r2 else 1) ^ (0 if p2 > b1 else 3), abs(p2 - b1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# mem_pestat
# ---------------------------------------------------------------------------------------------------------------------------------------
def cal_sub(opt, regs):
    """score of the first region that overlaps the best one on the query, or the score of a bare seed"""
    for r in regs[1:]:
        if _overlaps(r, regs[0], opt["mask_level"]):
            return r.score
    return opt["min_seed_len"] * opt["a"]


def pestat_candidates(regs_per_read, opt, l_pac):
    """sorted insert sizes per orientation of the pairs that vote: both ends aligned, both unique enough (cal_sub <= 0.8 of the best score), best hits on one
    contig, 0 < insert size <= max_ins"""
    isz = [[], [], [], []]
    for p in range(len(regs_per_read) // 2):
        r0, r1 = regs_per_read[2 * p], regs_per_read[2 * p + 1]
        if not r0 or not r1:
            continue
        if cal_sub(opt, r0) > F(0.8) * r0[0].score or cal_sub(opt, r1) > F(0.8) * r1[0].score:
            continue
        if r0[0].rid != r1[0].rid:
            continue
        d, dist = infer_dir(l_pac, r0[0].rb, r1[0].rb)
        if 0 < dist <= opt["max_ins"]:
            isz[d].append(dist)
    return [sorted(x) for x in isz]


def pestat(regs_per_read, opt, l_pac, sites=None):
    """four Pes (FF, FR, RF, RR) of one batch, as a definition over the sorted insert sizes of each orientation"""
    sites = sites if sites is not None else Sites()
    isz = pestat_candidates(regs_per_read, opt, l_pac)
    out = []
    for L in isz:
        n = len(L)
        if n < 10:
            out.append(Pes())
            continue
        p25, p75 = L[sites.trunc(F(0.25) * n)], L[sites.trunc(F(0.75) * n)]
        iqr = p75 - p25
        lo, hi = max(1, sites.trunc(F(p25 - 2 * iqr))), sites.trunc(F(p75 + 2 * iqr))
        core = [v for v in L if lo <= v <= hi]
        avg = F(sum(core), len(core))
        var = sum((v - avg) ** 2 for v in core) / len(core)
        std = MP.sqrt(MP.mpf(var.numerator) / var.denominator)
        mavg = MP.mpf(avg.numerator) / avg.denominator
        lo, hi = sites.trunc(F(p25 - 3 * iqr)), sites.trunc(F(p75 + 3 * iqr))
        if sites.compare_gt(lo, mavg - 4 * std):
            lo = sites.trunc(mavg - 4 * std)
        if sites.compare_gt(mavg + 4 * std, hi):
            hi = sites.trunc(mavg + 4 * std)
        out.append(Pes(max(1, lo), hi, 0, avg, std, len(core)))
    most = max(len(L) for L in isz)
    for L, r in zip(isz, out):
        if not r.failed and sites.compare_gt(most * F(0.05), len(L)):   # 0.05 as a double is above 1/20: at a count of exactly 5 % the product rounds to the count
            r.failed = 1                                   # low, high, avg, std stay as computed
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# mem_mark_primary_se (a second restatement: see the header)
# ---------------------------------------------------------------------------------------------------------------------------------------
def mark_primary(opt, regs, id_):
    """the list in the order (score descending, hash ascending) with sub, sub_n, secondary, secondary_all set; a new list of copies"""
    a = [r.copy() for r in regs]
    for i, r in enumerate(a):
        r.sub, r.secondary, r.secondary_all = 0, -1, -1
        r.hash = hash_64(id_ + i)
    a.sort(key=lambda r: (-r.score, r.hash))
    pen = _max_pen(opt)
    primaries = []
    for i, r in enumerate(a):
        if i == 0:
            primaries.append(0)
            continue
        for j in primaries:
            if _overlaps(a[j], r, opt["mask_level"]):
                if a[j].sub == 0:
                    a[j].sub = r.score
                if a[j].score - r.score <= pen:
                    a[j].sub_n += 1
                r.secondary = j
                break
        else:
            primaries.append(i)
    for r in a:
        r.secondary_all = r.secondary
    return a


# ---------------------------------------------------------------------------------------------------------------------------------------
# mem_approx_mapq_se
# ---------------------------------------------------------------------------------------------------------------------------------------
def _mpf(x):
    return MP.mpf(x.numerator) / x.denominator if isinstance(x, F) else MP.mpf(x)


def mapq_se(opt, r, sites=None):
    sites = sites if sites is not None else Sites()
    a, b = opt["a"], opt["b"]
    sub = r.sub if r.sub else opt["min_seed_len"] * a
    sub = max(sub, r.csub)
    if sub >= r.score:
        return 0
    l = max(r.qe - r.qb, r.re - r.rb)
    identity = 1 - F(l * a - r.score, a + b) / l
    if r.score == 0:
        mapq = 0
    elif opt["mapQ_coef_len"] > 0:
        k = F(6.02) * (r.score - sub) / a * identity ** 4
        if l < opt["mapQ_coef_len"]:
            mapq = sites.trunc(k)
        else:
            fac = opt["mapQ_coef_fac"]
            mapq = sites.trunc(lambda: _mpf(k) * (fac / MP.log(l)) ** 2, fast=float(k) * (fac / math.log(l)) ** 2)
    else:
        k = 30 * (1 - F(sub, r.score))
        mapq = sites.trunc(lambda: _mpf(k) * MP.log(r.seedcov), fast=float(k) * math.log(r.seedcov))
        if identity < F(0.95):
            mapq = sites.trunc(mapq * identity ** 2)
    if r.sub_n > 0:
        mapq -= sites.trunc(lambda: MP.mpf(4.343) * MP.log(r.sub_n + 1), fast=4.343 * math.log(r.sub_n + 1))
    mapq = min(60, max(0, mapq))
    return sites.trunc(mapq * (1 - F(r.frac_rep)))


def raw_mapq(opt, diff, sites):
    return sites.trunc(F(6.02) * diff / opt["a"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# mem_pair
# ---------------------------------------------------------------------------------------------------------------------------------------
SQRT1_2 = 0.70710678118654752440   # M_SQRT1_2 as the double it is


def pair_score(opt, s0, s1, dist, pes, sites):
    """q of one candidate: the two scores plus the log-probability of the insert size under the orientation's normal model, in units of a match"""
    ns = (dist - F(float(pes.avg))) / F(float(pes.std))        # the model as the doubles it is stored as
    arg = abs(ns) * F(SQRT1_2)

    def exact():
        p = 2 * MP.erfc(_mpf(arg))
        if p < MP.mpf(2) ** -1074:
            raise ArithmeticError("2 * erfc underflows in binary64: upstream's cast is undefined here (|ns| = %g)" % float(abs(ns)))
        return s0 + s1 + MP.mpf(0.721) * MP.log(p) * opt["a"]

    fa = float(arg)
    fast = s0 + s1 + 0.721 * math.log(2.0 * math.erfc(fa)) * opt["a"] if fa < 25 else None
    return max(0, sites.trunc(exact, fast=fast))


def pair(opt, regs0, regs1, pes, id_, l_pac, ctg_off, sites=None, info=None):
    """(o, sub, n_sub, z) of mem_pair over the two marked lists (all their regions are on the primary list: there are no ALT contigs here).
    The candidate SET: unordered pairs of a region of each read on one contig whose orientation class has not failed and whose distance on the forward strand
    lies in [low, high] of that class.  In the position order (forward-strand offset in the contig, then score, index, strand, read) the earlier region of a
    candidate is `k', the later `i'; the class is strand(k) * 2 + strand(i).  A candidate's key is (q, hash_64(rank(k) << 32 | rank(i) ^ id << 8) & 0xffffffff),
    its ranks breaking what is left.  o = the largest key's q, z = its regions; sub = the runner-up's q (0 without one); n_sub = the candidates other than the
    best with q >= sub - the largest single penalty.  info (a dict): receives the number of candidates, the largest q before the clamp at 0, and the ranks of
    the later region of the best and of the runner-up (what decides which lane of the wave form meets them), o, sub, n_sub, and the number of candidates
    exactly one largest penalty under the runner-up (the edge of the count)."""
    sites = sites if sites is not None else Sites()
    ends = []
    for r, regs in enumerate((regs0, regs1)):
        for i, e in enumerate(regs):
            strand = 1 if e.rb >= l_pac else 0
            pos = (e.rb if not strand else 2 * l_pac - 1 - e.rb) - ctg_off[e.rid]
            ends.append(((e.rid << 32 | pos), (e.score << 32 | i << 2 | strand << 1 | r), r, i, strand, e))
    ends.sort(key=lambda t: (t[0], t[1]))
    idw = id_ & 0xffffffff
    idw = idw - (1 << 32) if idw & 0x80000000 else idw          # (int)id
    sh = (idw << 8) & 0xffffffff
    sh = sh - (1 << 32) if sh & 0x80000000 else sh               # id << 8 in 32 bits, then sign-extended
    sh &= (1 << 64) - 1
    cands = []
    by_read = ([(rank, t) for rank, t in enumerate(ends) if t[2] == 0], [(rank, t) for rank, t in enumerate(ends) if t[2] == 1])
    for rk0, t0 in by_read[0]:
        for rk1, t1 in by_read[1]:
            if t0[5].rid != t1[5].rid:
                continue
            (rk, tk), (ri, ti) = ((rk0, t0), (rk1, t1)) if rk0 < rk1 else ((rk1, t1), (rk0, t0))
            d = tk[4] << 1 | ti[4]
            if pes[d].failed:
                continue
            dist = (ti[0] & 0xffffffff) - (tk[0] & 0xffffffff)
            if not pes[d].low <= dist <= pes[d].high:
                continue
            q = pair_score(opt, ti[5].score, tk[5].score, dist, pes[d], sites)
            y = rk << 32 | ri
            cands.append(((q, hash_64(y ^ sh) & 0xffffffff, y), tk, ti))
    if not cands:
        return 0, 0, 0, [0, 0]
    cands.sort(key=lambda c: c[0], reverse=True)
    best = cands[0]
    z = [0, 0]
    z[best[1][2]] = best[1][3]
    z[best[2][2]] = best[2][3]
    sub = cands[1][0][0] if len(cands) > 1 else 0
    n_sub = sum(1 for c in cands[1:] if sub - c[0][0] <= _max_pen(opt))
    if info is not None:
        info.update(n_cand=len(cands), best_rank=best[0][2] & 0xffffffff, second_rank=(cands[1][0][2] & 0xffffffff) if len(cands) > 1 else -1,
                    tied=len(cands) > 1 and cands[1][0][0] == best[0][0], n_equal_sub=sum(1 for c in cands if c[0][0] == sub),
                    o=best[0][0], sub=sub, n_sub=n_sub, n_at_edge=sum(1 for c in cands[1:] if sub - c[0][0] == _max_pen(opt)))
    return best[0][0], sub, n_sub, z


def pair_brute(opt, regs0, regs1, pes, id_, l_pac, ctg_off):
    """the same by walking the position-sorted list backwards from every region (tiny lists; the twin `pair' is checked against)"""
    v = []
    for r, regs in enumerate((regs0, regs1)):
        for i, e in enumerate(regs):
            st = int(e.rb >= l_pac)
            v.append((e.rid << 32 | ((e.rb if not st else 2 * l_pac - 1 - e.rb) - ctg_off[e.rid]), e.score << 32 | i << 2 | st << 1 | r))
    v.sort()
    sh = ((id_ << 8) & 0xffffffff)
    sh = (sh - (1 << 32) if sh >> 31 else sh) & ((1 << 64) - 1)
    u, s = [], Sites()
    for i in range(len(v)):
        for k in range(i - 1, -1, -1):
            if (v[k][1] & 1) == (v[i][1] & 1) or v[k][0] >> 32 != v[i][0] >> 32:
                continue
            d = (v[k][1] >> 1 & 1) << 1 | (v[i][1] >> 1 & 1)
            dist = v[i][0] - v[k][0]
            if pes[d].failed or dist < pes[d].low or dist > pes[d].high:
                continue
            q = pair_score(opt, v[i][1] >> 32, v[k][1] >> 32, dist, pes[d], s)
            u.append((q, hash_64((k << 32 | i) ^ sh) & 0xffffffff, k << 32 | i))
    if not u:
        return 0, 0, 0, [0, 0]
    u.sort()
    k, i = u[-1][2] >> 32, u[-1][2] & 0xffffffff
    z = [0, 0]
    z[v[i][1] & 1] = (v[i][1] & 0xffffffff) >> 2
    z[v[k][1] & 1] = (v[k][1] & 0xffffffff) >> 2
    sub = u[-2][0] if len(u) > 1 else 0
    return u[-1][0], sub, sum(1 for c in u[:-1] if sub - c[0] <= _max_pen(opt)), z


# ---------------------------------------------------------------------------------------------------------------------------------------
# mem_sam_pe's decision and the record list of mem_reg2sam
# ---------------------------------------------------------------------------------------------------------------------------------------
def _xa_owner(opt, a, j):
    k = a[j].secondary_all
    return k if k >= 0 and a[j].score >= a[k].score * F(opt["XA_drop_ratio"]) else -1


def _xa_records(opt, a, mains):
    """XA candidates: regions shadowed by a printed record whose score is within XA_drop_ratio of it, unless that record shadows more than max_XA_hits"""
    cnt = {}
    for j in range(len(a)):
        k = _xa_owner(opt, a, j)
        if k >= 0:
            cnt[k] = cnt.get(k, 0) + 1
    printed = {m[2] for m in mains if m[1] >= 0}
    out = []
    for j in range(len(a)):
        k = _xa_owner(opt, a, j)
        if k >= 0 and cnt[k] <= opt["max_XA_hits"] and cnt[k] <= opt["max_XA_hits_alt"] and k in printed:
            out.append((XA, j, k, 0, 0))
    return out


def decide(opt, a, pes, id_, l_pac, ctg_off, sites=None, info=None):
    """a = the two marked lists (modified as the stage leaves them: sub / secondary of a chosen secondary, secondary_all rewired).  Returns the records of
    the two reads: lists of (kind, region index in the marked list or -1, owner, flag, mapq), printed records first, then the XA candidates."""
    sites = sites if sites is not None else Sites()
    recs = [[], []]
    paired = False
    extra = 1
    o = sub = n_sub = 0
    z = [0, 0]
    if a[0] and a[1] and not opt["flag"] & F_NOPAIRING:
        o, sub, n_sub, z = pair(opt, a[0], a[1], pes, id_, l_pac, ctg_off, sites, info)
    if a[0] and a[1] and o > 0:
        multi = [any(r.secondary < 0 and r.score >= opt["T"] for r in a[i][1:]) for i in range(2)]
        if not any(multi):
            paired = True
            if info is not None:
                info["branch"] = "paired"
            score_un = a[0][0].score + a[1][0].score - opt["pen_unpaired"]
            sub = max(sub, score_un)
            q_pe = raw_mapq(opt, o - sub, sites)
            if n_sub > 0:
                q_pe -= sites.trunc(lambda: MP.mpf(4.343) * MP.log(n_sub + 1), fast=4.343 * math.log(n_sub + 1))
            q_pe = min(60, max(0, q_pe))
            fsum = F(float(np.float32(a[0][0].frac_rep) + np.float32(a[1][0].frac_rep)))
            q_pe = sites.trunc(q_pe * (1 - F(0.5) * fsum))
            if o > score_un:
                q_se = []
                for i in range(2):
                    c = a[i][z[i]]
                    if c.secondary >= 0:
                        c.sub, c.secondary = a[i][c.secondary].score, -2
                    q = mapq_se(opt, c, sites)
                    q = q if q > q_pe else min(q_pe, q + 40)
                    q_se.append(min(q, raw_mapq(opt, c.score - c.csub, sites)))
                extra |= 2
            else:
                z = [0, 0]
                q_se = [mapq_se(opt, a[0][0], sites), mapq_se(opt, a[1][0], sites)]
            for i in range(2):
                k = a[i][z[i]].secondary_all
                if k >= 0:
                    for j, r in enumerate(a[i]):
                        if r.secondary_all == k or j == k:
                            r.secondary_all = z[i]
                    a[i][z[i]].secondary_all = -1
                recs[i].append((MAIN, z[i], z[i], (0x40 << i) | extra, q_se[i]))
    if not paired:
        if a[0] and a[1] and a[0][0].score >= opt["T"] and a[1][0].score >= opt["T"] and a[0][0].rid == a[1][0].rid:
            d, dist = infer_dir(l_pac, a[0][0].rb, a[1][0].rb)
            if not pes[d].failed and pes[d].low <= dist <= pes[d].high:
                extra |= 2
        for i in range(2):
            first_q = None
            for k, r in enumerate(a[i]):
                if r.score < opt["T"] or r.secondary >= 0:
                    continue
                q = mapq_se(opt, r, sites)
                flag = (0x81 if i else 0x41) | extra
                if first_q is None:
                    first_q = q
                else:
                    flag |= 0x10000 if opt["flag"] & F_NO_MULTI else 0x800
                    q = min(q, first_q)
                recs[i].append((MAIN, k, k, flag, q))
            if first_q is None:
                recs[i].append((MAIN, -1, -1, (0x81 if i else 0x41) | extra | 0x4, 0))
    for i in range(2):
        recs[i] += _xa_records(opt, a[i], recs[i])
    return recs


def pair_final(opt, regs0, regs1, pes, pair_id, l_pac, ctg_off, sites=None, info=None):
    """the whole stage for one pair (pair_id = ordinal of the pair in the input): (marked lists as the stage leaves them, records per read)"""
    a = [mark_primary(opt, regs0, pair_id << 1 | 0), mark_primary(opt, regs1, pair_id << 1 | 1)]
    recs = decide(opt, a, pes, pair_id, l_pac, ctg_off, sites, info)
    return a, recs
