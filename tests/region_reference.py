"""Independent reference of the region stage (upstream mem_chain2aln for every chain of a read, then mem_sort_dedup_patch with mem_patch_reg; SURVEY.md 8a
rows a6 and a8) -- TEST INFRASTRUCTURE ONLY.

Written from SURVEY.md Appendix B and upstream's documented behaviour (bwamem.c), not from csrc/k_extend.h, csrc/k_extlane.h, csrc/k_sdp.h or
oracle/orc_mem.c.  It imports neither oracle_py nor speedseq_amd.capi and shares with them the option names and nothing else: no packed key, no bin, no
lane, no slab.  Integers, fractions.Fraction, Python floats (IEEE binary64, the type of upstream's `double'), lists and sets.  The two DP operations come
from tests/dp_reference.py, which is pinned on its own: `extend' for both sides of a seed, `global_' for mem_patch_reg.  The reference text comes from the
2-bit pac as matesw_reference.Ref reads it: doubled coordinates, position p >= l_pac the complement of 2 l_pac - 1 - p, and bns_fetch_seq's cut to the
contig and strand of the chain's first seed.

What is a DEFINITION here (a closed expression or a set, no loop that stops early):
  * cal_max_gap   the longest gap a stretch of qlen matching bases pays for, per gap kind, the larger, at least 1, capped at 2 w;
  * window        the union over the chain's seeds of the per-seed interval, clamped to [0, 2 l_pac), cut at l_pac by the first seed's strand, cut to its contig;
  * seedcov       the sum of len over the SET of the chain's seeds that lie inside the region on both axes;
  * local vs to-end  the rule on the extension's results: to-end only when gscore > 0 and gscore > score - pen_clip;
  * w             max(aw0, aw1), the bands the two sides ended on.
What is a SECOND RESTATEMENT (greedy and order dependent: the loop again, in another hand):
  * the visiting order (score << 32 | i, highest first) -- stated as a sort by (score, index), descending;
  * the containment test with its off-diagonal walk over the seeds of higher rank and the `srt[i] = 0' marks;
  * the band retry (at most two tries, left when the score repeats or max_off stays below 3/4 of the band);
  * the redundancy scan of mem_sort_dedup_patch with its side effects (a region emptied in mid-scan is skipped by the scans after it);
  * mem_patch_reg with the band of bwa_gen_cigar2;
  * the identical-hit pass after the second sort.

Real numbers.  Every comparison in real numbers is evaluated twice: exactly (Fractions; a constant written as a decimal in upstream's source enters at the value
of its C type) and in the type upstream uses.  The upstream type decides; a site where the two part is a NEAR site, counted in the Tally:
  * s.len - seedlen0 > .1 * l_query                 binary64 product;
  * t.len < s.len * .95                             binary64 product;
  * or > mask_level_redun * mr (and oq, mq)         binary32 product of the option's binary32 value and an integer below 2^24;
  * r >= 0.05f, r >= 0.05f * 2                      r in binary64 (two divisions and a subtraction), the bound a binary32 constant;
  * (double)score / max(q_s, r_s) < 0.90f           binary64 quotient against a binary32 constant;
  * q_s, r_s = (int)(x + .499)                      binary64 quotient, product and sum, truncated.
For the exact side the constants are the values the C types hold (0.1 and 0.95 as binary64, 0.05f and 0.90f as binary32), so that a site parts only
where the ROUNDING OF AN OPERATION decides, which is what a build with other arithmetic (a fused multiply-add, a float where a double stood) would change.
The site that shows it: 0.95f x 20 is 18.99999976 before the product is rounded and 19.0 after, so an overlap of 19 on a shorter side of 20 is redundant exactly
and NOT redundant upstream; `near_redun' counts it, and every build has to take the binary32 side.

Where the answer is not decided here.  Both sorts of mem_sort_dedup_patch are unstable upstream (ks_introsort).  Where keys tie -- `re' in the first sort,
(score, rb, qb) in the second -- `sort_dedup_patch' evaluates every order of each tie group, for groups of up to 4 and at most MAX_ORDERS orders in all.  If
all orders give the same list, that list is the answer; otherwise, and for larger groups, the read is ORDER-DEPENDENT: `regions' returns None for its list
and the tests compare such a read with the oracle only.
"""
import itertools
from fractions import Fraction as F

import dp_reference as dp
from chain_reference import f32

FIELDS = ("rb", "re", "qb", "qe", "rid", "score", "truesc", "sub", "alt_sc", "csub", "sub_n", "w", "seedcov", "secondary", "secondary_all", "seedlen0", "n_comp",
          "frac_rep", "hash")
DEFAULTS = dict(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, w=100, zdrop=100, pen_clip5=5, pen_clip3=5, max_chain_gap=10000, mask_level_redun=0.95)
MAX_TIE, MAX_ORDERS = 4, 600
D_01, D_095 = F(0.1), F(0.95)                          # the binary64 values of upstream's `.1' and `.95'
F_005, F_090 = f32(F(5, 100)), f32(F(90, 100))         # the binary32 values of PATCH_MAX_R_BW and PATCH_MIN_SC_RATIO


class Tally:
    """what a run met: counts by name (near sites `near_*', band retries, patches, tie groups, order-dependent reads)"""

    def __init__(self):
        self.c = {}

    def add(self, k, n=1):
        self.c[k] = self.c.get(k, 0) + n

    def __getitem__(self, k):
        return self.c.get(k, 0)

    def near(self):
        return sum(v for k, v in self.c.items() if k.startswith("near_"))


def opt_from(rec=None, **kw):
    """the option values this stage reads, from a record with those field names or the defaults, then kw; mask_level_redun enters at its binary32 value"""
    o = dict(DEFAULTS)
    if rec is not None:
        for k in DEFAULTS:
            o[k] = rec[k].item() if hasattr(rec[k], "item") else rec[k]
    o.update(kw)
    o["mask_level_redun"] = f32(F(o["mask_level_redun"]))
    return o


def scores_of(opt):
    return (opt["a"], opt["b"], opt["o_del"], opt["e_del"], opt["o_ins"], opt["e_ins"])


class Ref:
    """the doubled reference: forward bases from the 2-bit pac (base k in byte k >> 2 at bits (~k & 3) * 2), contigs that tile [0, l_pac)"""

    def __init__(self, pac, l_pac, ctg_off, ctg_len):
        self.pac, self.l_pac, self.ctg_off, self.ctg_len = pac, int(l_pac), [int(x) for x in ctg_off], [int(x) for x in ctg_len]

    def _fwd(self, k):
        return (int(self.pac[k >> 2]) >> ((~k & 3) << 1)) & 3

    def base(self, p):
        return self._fwd(p) if p < self.l_pac else 3 - self._fwd(2 * self.l_pac - 1 - p)

    def bases(self, rb, re):
        return [self.base(p) for p in range(rb, re)]

    def rid_of(self, pos):
        f = pos if pos < self.l_pac else 2 * self.l_pac - 1 - pos
        for i in range(len(self.ctg_off)):
            if self.ctg_off[i] <= f < self.ctg_off[i] + self.ctg_len[i]:
                return i
        raise ValueError("position %d outside the contigs" % pos)

    def contig_span(self, pos):
        """the doubled-coordinate interval of the contig and strand that hold pos"""
        rid = self.rid_of(pos)
        beg, end = self.ctg_off[rid], self.ctg_off[rid] + self.ctg_len[rid]
        if pos >= self.l_pac:
            beg, end = 2 * self.l_pac - end, 2 * self.l_pac - beg
        return beg, end, rid


def trunc(x):
    """C's conversion of a real to int: toward zero"""
    x = F(x)
    return int(x) if x >= 0 else -int(-x)


def cal_max_gap(opt, qlen):
    """DEFINITION.  (qlen * a - o) / e + 1 truncated, per gap kind; the larger; at least 1; at most 2 w.  (The quotient of two small integers plus one never
    lies within a binary64 rounding of an integer it does not equal, so the exact value is upstream's.)"""
    l_del = trunc(F(qlen * opt["a"] - opt["o_del"], opt["e_del"]) + 1)
    l_ins = trunc(F(qlen * opt["a"] - opt["o_ins"], opt["e_ins"]) + 1)
    return min(max(l_del, l_ins, 1), opt["w"] << 1)


def window(opt, ref, l_query, seeds):
    """DEFINITION.  seeds: (rbeg, qbeg, len) of the chain in chain order.  (rmax0, rmax1, rid)"""
    lo = min(rb - (qb + cal_max_gap(opt, qb)) for rb, qb, ln in seeds)
    hi = max(rb + ln + (l_query - qb - ln) + cal_max_gap(opt, l_query - qb - ln) for rb, qb, ln in seeds)
    lo, hi = max(lo, 0), min(hi, 2 * ref.l_pac)
    first = seeds[0][0]
    if lo < ref.l_pac < hi:
        if first < ref.l_pac:
            hi = ref.l_pac
        else:
            lo = ref.l_pac
    beg, end, rid = ref.contig_span(first)
    return max(lo, beg), min(hi, end), rid


def seedcov(seeds, a):
    """DEFINITION.  the sum of len over the set of seeds inside the region on both axes"""
    inside = {i for i, (rb, qb, ln) in enumerate(seeds) if qb >= a["qb"] and qb + ln <= a["qe"] and rb >= a["rb"] and rb + ln <= a["re"]}
    return sum(seeds[i][2] for i in inside)


def to_end(gscore, score, pen_clip):
    """DEFINITION.  the extension is taken to the end of the query only when reaching it scored, and scored more than the local maximum less the clipping penalty"""
    return gscore > 0 and gscore > score - pen_clip


def _gt_prod64(lhs, c, n, tally, name):
    """lhs > c * n with c a binary64 constant (given as its exact Fraction) and the product rounded to binary64, as C evaluates it; the exact form is tallied"""
    c_form = lhs > float(c) * n
    if c_form != (lhs > c * n):
        tally.add(name)
    return c_form


def _lt_prod64(lhs, c, n, tally, name):
    c_form = lhs < n * float(c)
    if c_form != (lhs < c * n):
        tally.add(name)
    return c_form


def contained(opt, l_query, s, p, tally):
    """SECOND RESTATEMENT.  is seed s = (rbeg, qbeg, len) inside region p and near one of its end diagonals?"""
    rb, qb, ln = s
    if rb < p["rb"] or rb + ln > p["re"] or qb < p["qb"] or qb + ln > p["qe"]:
        return False
    if _gt_prod64(ln - p["seedlen0"], D_01, l_query, tally, "near_seedlen"):
        return False
    for qd, rd in ((qb - p["qb"], rb - p["rb"]), (p["qe"] - (qb + ln), p["re"] - (rb + ln))):
        w = min(cal_max_gap(opt, min(qd, rd)), p["w"])
        if qd - rd < w and rd - qd < w:
            return True
    return False


def off_diagonal(s, t, tally):
    """SECOND RESTATEMENT.  does the higher-ranked seed t overlap s by a quarter of s and more, off s's diagonal?  (a seed shorter than .95 of s is not asked)"""
    srb, sqb, sln = s
    trb, tqb, tln = t
    if _lt_prod64(tln, D_095, sln, tally, "near_walk"):
        return False
    if sqb <= tqb and sqb + sln - tqb >= sln >> 2 and tqb - sqb != trb - srb:
        return True
    if tqb <= sqb and tqb + tln - sqb >= sln >> 2 and sqb - tqb != srb - trb:
        return True
    return False


def extend_side(opt, q, t, h0, pen_clip, before, tally):
    """SECOND RESTATEMENT of the band retry around dp_reference.extend: (result of the last try, the band it ran in).  At most two tries, the second in twice the
    band; a try is the last when its score is the one held before it (`before': the region's score when the side starts, -1 on the left, the left side's on the
    right) or when the best cell strayed less than 3/4 of the band from the diagonal."""
    score, res, aw = before, None, opt["w"]
    for i in range(2):
        prev, aw = score, opt["w"] << i
        res = dp.extend(q, t, scores_of(opt), aw, pen_clip, opt["zdrop"], h0)
        score = res[0]
        if score == prev or res[5] < (aw >> 1) + (aw >> 2):
            break
        if i == 0:
            tally.add("retry")
    if opt.get("count_zdrop") and opt["zdrop"] > 0:
        # did the z-drop end this side?  The same extension without it fills more rows.  (Asked for by a test that is built for it: it doubles the DP.)
        filled = lambda H: sum(1 for i in range(1, H.shape[0]) if H[i][1:].any())
        with_z = dp.extend(q, t, scores_of(opt), aw, pen_clip, opt["zdrop"], h0, matrices=True)[1][0]
        without = dp.extend(q, t, scores_of(opt), aw, pen_clip, 0, h0, matrices=True)[1][0]
        if filled(with_z) < filled(without):
            tally.add("zdrop_ended")
    return res, aw


def chain2aln(opt, ref, query, seeds, rid, frac_rep, av, tally):
    """mem_chain2aln for one chain: appends its regions to av.  seeds: (rbeg, qbeg, len) in chain order; the score of a seed is its len."""
    l_query = len(query)
    rmax0, rmax1, rid_w = window(opt, ref, l_query, seeds)
    assert rid_w == rid, "the chain's rid is not the contig of its first seed"
    rseq = ref.bases(rmax0, rmax1)
    order = sorted(range(len(seeds)), key=lambda i: (seeds[i][2], i))          # ascending; visited from the end
    marked = [False] * len(order)
    for k in range(len(order) - 1, -1, -1):
        s = seeds[order[k]]
        rb, qb, ln = s
        # (the box test stands here as well as in `contained': a read of two thousand regions asks four million times, nearly always in vain)
        if any(rb >= p["rb"] and rb + ln <= p["re"] and qb >= p["qb"] and qb + ln <= p["qe"] and contained(opt, l_query, s, p, tally) for p in av):
            # a seed already covered is dropped unless a live seed of higher rank crosses it off its diagonal
            if not any(off_diagonal(s, seeds[order[i]], tally) for i in range(k + 1, len(order)) if not marked[i]):
                marked[k] = True
                continue
        a = dict.fromkeys(FIELDS, 0)
        a["rid"], a["frac_rep"], a["seedlen0"] = rid, frac_rep, ln
        aw0 = aw1 = opt["w"]
        if qb:
            tmp = rb - rmax0
            res, aw0 = extend_side(opt, query[:qb][::-1], rseq[:tmp][::-1], ln * opt["a"], opt["pen_clip5"], -1, tally)
            score, qle, tle, gtle, gscore, _ = res
            if to_end(gscore, score, opt["pen_clip5"]):
                a["qb"], a["rb"], a["truesc"] = 0, rb - gtle, gscore
                tally.add("to_end")
            else:
                a["qb"], a["rb"], a["truesc"] = qb - qle, rb - tle, score
            if gscore > 0 and gscore == score - opt["pen_clip5"]:
                tally.add("edge_gscore")
            a["score"] = score
        else:
            a["score"] = a["truesc"] = ln * opt["a"]
            a["qb"], a["rb"] = 0, rb
        if qb + ln != l_query:
            qe, re, sc0 = qb + ln, rb + ln - rmax0, a["score"]
            res, aw1 = extend_side(opt, query[qe:], rseq[re:], sc0, opt["pen_clip3"], sc0, tally)
            score, qle, tle, gtle, gscore, _ = res
            if to_end(gscore, score, opt["pen_clip3"]):
                a["qe"], a["re"] = l_query, rmax0 + re + gtle
                a["truesc"] += gscore - sc0
                tally.add("to_end")
            else:
                a["qe"], a["re"] = qe + qle, rmax0 + re + tle
                a["truesc"] += score - sc0
            if gscore > 0 and gscore == score - opt["pen_clip3"]:
                tally.add("edge_gscore")
            a["score"] = score
        else:
            a["qe"], a["re"] = l_query, rb + ln
        a["seedcov"] = seedcov(seeds, a)
        a["w"] = max(aw0, aw1)
        av.append(a)


# ------------------------------------------------------------------------------------------------------------------------------
# mem_sort_dedup_patch
# ------------------------------------------------------------------------------------------------------------------------------
def _f32_gt(lhs, m, n, tally, name):
    """lhs > m * n in binary32: m the option's binary32 value, n and lhs integers that convert exactly"""
    assert abs(lhs) < 1 << 24 and abs(n) < 1 << 24
    c_form = lhs > f32(m * n)
    if c_form != (lhs > m * n):
        tally.add(name)
    return c_form


def redundant(opt, p, q, tally):
    """SECOND RESTATEMENT.  p ends at or after q: do they cover one another beyond mask_level_redun of the shorter, on the reference and on the query?"""
    m = opt["mask_level_redun"]
    or_ = q["re"] - p["rb"]
    oq = q["qe"] - p["qb"] if q["qb"] < p["qb"] else p["qe"] - q["qb"]
    mr = min(q["re"] - q["rb"], p["re"] - p["rb"])
    mq = min(q["qe"] - q["qb"], p["qe"] - p["qb"])
    return _f32_gt(or_, m, mr, tally, "near_redun") and _f32_gt(oq, m, mq, tally, "near_redun")


def gen_band(opt, l_query, rlen, w_):
    """the band bwa_gen_cigar2 runs ksw_global2 in: what half the query pays for plus the length difference, halved; at most w_; at least |difference| + 3"""
    max_ins = trunc(F(((l_query + 1) >> 1) * opt["a"] - opt["o_ins"], opt["e_ins"]) + 1)
    max_del = trunc(F(((l_query + 1) >> 1) * opt["a"] - opt["o_del"], opt["e_del"]) + 1)
    max_gap = max(max_ins, max_del, 1)
    w = min((max_gap + abs(rlen - l_query) + 1) >> 1, w_)
    return max(w, abs(rlen - l_query) + 3)


def patch_reg(opt, ref, query, a, b, tally):
    """SECOND RESTATEMENT of mem_patch_reg: (score, w) of the alignment that joins a (the earlier on the reference) and b, or (0, reason)"""
    assert a["rid"] == b["rid"] and a["rb"] <= b["rb"]
    if a["rb"] < ref.l_pac <= b["rb"]:
        return 0, "strands"
    if a["qb"] >= b["qb"] or a["qe"] >= b["qe"] or a["re"] >= b["re"]:
        return 0, "not colinear"
    w = abs((a["re"] - b["rb"]) - (a["qe"] - b["qb"]))
    x1, x2 = F(a["re"] - b["rb"], b["re"] - a["rb"]), F(a["qe"] - b["qb"], b["qe"] - a["qb"])
    r_c = abs(float(a["re"] - b["rb"]) / (b["re"] - a["rb"]) - float(a["qe"] - b["qb"]) / (b["qe"] - a["qb"]))
    r_x = abs(x1 - x2)
    gap = a["re"] < b["rb"] or a["qe"] < b["qb"]
    bound = F_005 if gap else 2 * F_005              # (0.05f * 2 is exact in binary32)
    if (r_c >= float(bound)) != (r_x >= bound):
        tally.add("near_patch_r")
    if w > opt["w"] << (1 if gap else 2):
        return 0, "w"
    if r_c >= float(bound):
        return 0, "r"
    w = min(w + a["w"] + b["w"], opt["w"] << 2)
    tally.add("patch_aligned")
    rb, re, qb, qe = a["rb"], b["re"], a["qb"], b["qe"]
    if qe - qb <= 0 or rb >= re or rb < ref.l_pac < re or rb < 0 or re > 2 * ref.l_pac:
        score = 0                                     # (bwa_gen_cigar2 returns without a score: upstream's is whatever `score' held; regions never get here)
    else:
        q, t = list(query[qb:qe]), ref.bases(rb, re)
        if qe - qb == re - rb and w == 0:
            score = sum(dp._sub1(scores_of(opt), t[i], q[i]) for i in range(len(q)))
        else:
            score = dp.global_(q, t, scores_of(opt), gen_band(opt, qe - qb, re - rb, w))
    tot = b["score"] + a["score"]
    est = []
    for num, den in ((b["qe"] - a["qb"], (b["qe"] - b["qb"]) + (a["qe"] - a["qb"])), (b["re"] - a["rb"], (b["re"] - b["rb"]) + (a["re"] - a["rb"]))):
        c_form = int(float(num) / den * tot + .499)
        if c_form != trunc(F(num, den) * tot + F(.499)):
            tally.add("near_patch_est")
        est.append(c_form)
    top = max(est)
    assert top > 0
    c_form = float(score) / top < float(F_090)
    if c_form != (F(score, top) < F_090):
        tally.add("near_patch_ratio")
    if c_form:
        return 0, "ratio"
    return score, w


def _scan(opt, ref, query, a, tally):
    """the redundancy scan over a list sorted by re, with its side effects; then the compaction"""
    for x in a:
        x["n_comp"] = 1
    for i in range(1, len(a)):
        p = a[i]
        if p["rid"] != a[i - 1]["rid"] or p["rb"] >= a[i - 1]["re"] + opt["max_chain_gap"]:
            continue
        j = i - 1
        while j >= 0 and p["rid"] == a[j]["rid"] and p["rb"] < a[j]["re"] + opt["max_chain_gap"]:
            q = a[j]
            j -= 1
            if q["qe"] == q["qb"]:
                continue
            if redundant(opt, p, q, tally):
                tally.add("redundant")
                if p["score"] < q["score"]:
                    p["qe"] = p["qb"]
                    break
                q["qe"] = q["qb"]
            elif q["rb"] < p["rb"]:
                tally.add("patch_tried")
                score, w = patch_reg(opt, ref, query, q, p, tally)
                if score <= 0:
                    tally.add("patch_no_%s" % (w if isinstance(w, str) else "score"))
                if score > 0:
                    tally.add("patched")
                    p["n_comp"] += q["n_comp"] + 1
                    for f in ("seedcov", "sub", "csub"):
                        p[f] = max(p[f], q[f])
                    p["qb"], p["rb"] = q["qb"], q["rb"]
                    p["truesc"] = p["score"] = score
                    p["w"] = w
                    q["qb"] = q["qe"]
    return [x for x in a if x["qe"] > x["qb"]]


def _orders(items, key):
    """every order of `items' that a sort by `key' may leave: the tie groups permuted; None when a group or the product is beyond the caps"""
    items = sorted(items, key=key)
    groups = [list(g) for _, g in itertools.groupby(items, key=key)]
    n = 1
    for g in groups:
        if len(g) > MAX_TIE:
            return None
        for k in range(2, len(g) + 1):
            n *= k
        if n > MAX_ORDERS:
            return None
    return ([x for g in combo for x in g] for combo in itertools.product(*[list(itertools.permutations(g)) for g in groups]))


def _copy(lst):
    return [dict(x) for x in lst]


def sort_dedup_patch(opt, ref, query, regs, tally=None):
    """mem_sort_dedup_patch: the list, or None where the outcome depends on what an unstable sort does with equal keys (see the head of this file)"""
    tally = tally if tally is not None else Tally()
    if len(regs) <= 1:
        return _copy(regs)
    first = _orders(regs, lambda x: x["re"])
    if first is None:
        tally.add("ties_beyond_caps")
        return None
    answer, n_orders = None, 0
    for k1, o1 in enumerate(first):
        t = tally if k1 == 0 else Tally()             # the counts of the first order stand for the read
        left = _scan(opt, ref, query, _copy(o1), t)
        second = _orders(left, lambda x: (-x["score"], x["rb"], x["qb"]))
        if second is None:
            tally.add("ties_beyond_caps")
            return None
        for o2 in second:
            n_orders += 1
            if n_orders > MAX_ORDERS:
                tally.add("ties_beyond_caps")
                return None
            o2 = _copy(o2)
            for i in range(1, len(o2)):               # identical hits: the later one of an equal (score, rb, qb) goes
                if (o2[i]["score"], o2[i]["rb"], o2[i]["qb"]) == (o2[i - 1]["score"], o2[i - 1]["rb"], o2[i - 1]["qb"]):
                    o2[i]["qe"] = o2[i]["qb"]
            out = o2[:1] + [x for x in o2[1:] if x["qe"] > x["qb"]]
            if answer is None:
                answer = out
            elif out != answer:
                tally.add("order_dependent")
                return None
    if n_orders > 1:
        tally.add("tie_reads_decided")
    return answer


def regions(opt, ref, query, chains, tally=None):
    """the stage for one read.  chains: [(rid, frac_rep, [(rbeg, qbeg, len), ...]), ...] in the chaining stage's order.
    (list of regions or None when order-dependent, the regions before mem_sort_dedup_patch)"""
    tally = tally if tally is not None else Tally()
    query = [int(c) for c in query]
    av = []
    for rid, frac_rep, seeds in chains:
        chain2aln(opt, ref, query, [tuple(int(v) for v in s) for s in seeds], int(rid), float(frac_rep), av, tally)
    return sort_dedup_patch(opt, ref, query, av, tally), av
