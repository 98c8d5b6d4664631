"""Independent reference of the record stage (upstream mem_reg2aln -> bwa_gen_cigar2 -> ksw_global2, NM and MD) -- TEST INFRASTRUCTURE ONLY.

Written from SURVEY.md Appendix B and oracle/README.md rows 9a-9c, not from csrc/k_aln.h, csrc/k_sw.h or oracle/orc_pair.c.  It imports neither oracle_py nor
speedseq_amd.capi and shares with them the field names and nothing else: no packed cell, no ring, no direction nibble, no lane.  Plain Python integers and
lists.  The banded optimum comes from dp_reference.global_ and the walk of a CIGAR from dp_reference.rescore, both pinned on their own; the band of
bwa_gen_cigar2 is region_reference.gen_band, the one statement of it in the tests; the reference text is region_reference.Ref.

The alignment is always stated ON THE FORWARD STRAND.  A region of the reverse strand (rb >= l_pac) covers forward bases [2 l_pac - re, 2 l_pac - rb); the read's
piece [qb, qe) enters as its reverse complement (an N stays an N), the reference as the forward text.  That is what upstream reaches by reversing both sequences
before ksw_global2, and it makes "leftmost" mean one thing for both strands.

What is a DEFINITION here (a closed expression, a set, or an optimum that is unique):
  * infer_bw        0 when the lengths are equal and l a - score < 2 (o + e - a); else (min(l1, l2) a - score - o) / e + 2 truncated, at least |l1 - l2|;
  * w2              the larger infer_bw of deletion and insertion; min'ed with the region's w only when above opt.w; at most opt.w << 2;
  * the band        region_reference.gen_band;
  * the gap-free branch   equal lengths and w2 = 0: one M, the score the sum over the columns;
  * the retry       `rounds': the sequence of (w2, band, optimal score): it ends when the score repeats, when w2 is opt.w << 2, after three rounds, or when
                    score >= truesc - a;
  * the CIGAR's properties   for the band the retry ends on: consumes query and window whole, stays in the band, earns the optimum (dp_reference.rescore against
                    dp_reference.global_), no zero-length op, no two equal neighbours -- `check_cigar';
  * a unique optimum   `n_paths' counts the optimal paths of the band over (row, column, state M / D / I), gaps opening from a diagonal step only; where it is 1 the
                    CIGAR is forced;
  * a single gap in a repeat   the leftmost placement on the forward strand, for regions of either strand -- `leftmost_single_gap' finds it by trying every place;
  * the squeeze     one leading deletion is removed and POS moved by it, else one trailing deletion is removed; never both;
  * clips           in forward-strand order: the read's unaligned 5' end is the left clip on the forward strand and the right clip on the reverse strand;
  * POS, rid        the forward coordinate of rb (forward strand) or of re - 1 (reverse strand), plus a removed leading deletion; rid the contig of that position;
  * flag, mapq, score, sub, reg_idx   copied: flag | 0x100 for a secondary region, sub = max(sub, csub), reg_idx = the request's owner;
  * NM, MD          from the CIGAR and the bases alone: a query N always mismatches; inserted bases count; deleted bases count, and appear in MD, only between two
                    other ops; letters are forward-strand bases.  Self-check `rebuild': read + CIGAR + MD give back the forward text at POS.
What is a SECOND RESTATEMENT (the loop again, in another hand):
  * the choice among tied optimal paths: walking back from the last cell, a diagonal step before a deletion before an insertion, and a gap that may either open or
    extend at equal score opens.  Where n_paths > 1 and the record is no single gap in a repeat, this order is all that stands behind the CIGAR; `ties_met'
    counts, on the path taken, the cells where two (h) or all three (h3) states tie and the gaps that could open or extend (oe).

Cell extremes.  `record' reports lo / hi: the extreme values over every reachable in-band M, D and I cell and every gap-opening candidate M - (o + e) of the band the
retry ends on, and lo_first / hi_first of the first band (the one the lane DP runs).  A kernel that keeps cells in fewer bits can be judged against them without
being run.
"""
import dp_reference as dp
from region_reference import Ref, gen_band, scores_of, trunc  # noqa: F401  (Ref is re-exported for the tests)
from fractions import Fraction as F

NEG = dp.NEG
REACH = NEG // 2          # above it: a value of a reachable cell
DEFAULTS = dict(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, w=100)
FIELDS = ("pos", "rid", "flag", "mapq", "NM", "score", "sub", "n_cigar", "is_rev", "l_md", "reg_idx", "xa_cnt", "kind", "cigar", "md")
MAX_CIGAR, MAX_MD, Z_CAP = 64, 320, 192 * 1024     # the layout of ssg_aln_t and the wave kernel's direction slab (include/ssgpu.h: documented capacities)


def opt_from(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def infer_bw(l1, l2, score, a, q, r):
    """DEFINITION.  The band a local score implies for one gap kind (open q, extend r)."""
    if l1 == l2 and l1 * a - score < (q + r - a) << 1:
        return 0
    return max(trunc(F(min(l1, l2) * a - score - q, r) + 2), abs(l1 - l2))


def w2_of(opt, qlen, tlen, truesc, reg_w):
    """DEFINITION.  The band mem_reg2aln starts from (before the cap at opt.w << 2, which `rounds' applies each round)."""
    w2 = max(infer_bw(qlen, tlen, truesc, opt["a"], opt["o_del"], opt["e_del"]), infer_bw(qlen, tlen, truesc, opt["a"], opt["o_ins"], opt["e_ins"]))
    if w2 > opt["w"]:
        w2 = min(w2, reg_w)
    return w2


def sub1(opt, tb, qb):
    return -1 if tb > 3 or qb > 3 else opt["a"] if tb == qb else -opt["b"]


def rounds(opt, qa, ta, w2, truesc):
    """DEFINITION.  The retry loop as [(w2, band or None for the gap-free branch, optimal score)]."""
    out, last, i = [], None, 0
    cap = opt["w"] << 2
    while True:
        w2 = min(w2, cap)
        if len(qa) == len(ta) and w2 == 0:
            band, score = None, sum(sub1(opt, t, q) for t, q in zip(ta, qa))
        else:
            band = gen_band(opt, len(qa), len(ta), w2)
            score = dp.global_(qa, ta, scores_of(opt), band)
        out.append((w2, band, score))
        if score == last or w2 == cap:
            break
        last = score
        w2 <<= 1
        i += 1
        if not (i < 3 and score < truesc - opt["a"]):
            break
    return out


def band_dp(opt, qa, ta, w):
    """the band over (row, column, state), 1-based with a boundary row and column: matrices M, D, I as dicts of in-band cells, the optimal score, the number of optimal
    paths and the extremes (lo, hi) of every reachable value and gap-opening candidate"""
    a, b, o_del, e_del, o_ins, e_ins = scores_of(opt)
    n, m = len(ta), len(qa)
    M, D, I, H, C = {}, {}, {}, {}, {}        # C: optimal paths into (state, i, j)
    lo, hi = 0, 0

    def see(v):
        nonlocal lo, hi
        if v > REACH:
            lo, hi = min(lo, v), max(hi, v)
    H[(0, 0)] = 0; C[("H", 0, 0)] = 1
    for j in range(1, min(m, w) + 1):
        H[(0, j)] = -(o_ins + e_ins * j); C[("H", 0, j)] = 1; see(H[(0, j)])
    for i in range(1, min(n, w) + 1):
        H[(i, 0)] = -(o_del + e_del * i); C[("H", i, 0)] = 1; see(H[(i, 0)])
    for i in range(1, n + 1):
        for j in range(max(1, i - w), min(m, i + w) + 1):
            d = H.get((i - 1, j - 1), NEG)
            mv = d + sub1(opt, ta[i - 1], qa[j - 1]) if d > REACH else NEG
            cm = C.get(("H", i - 1, j - 1), 0) if d > REACH else 0
            e1, e2 = D.get((i - 1, j), NEG), M.get((i - 1, j), NEG)
            e1 = e1 - e_del if e1 > REACH else NEG
            e2 = e2 - (o_del + e_del) if e2 > REACH else NEG
            dv = max(e1, e2)
            cd = (C.get(("D", i - 1, j), 0) if e1 == dv else 0) + (C.get(("M", i - 1, j), 0) if e2 == dv else 0) if dv > REACH else 0
            f1, f2 = I.get((i, j - 1), NEG), M.get((i, j - 1), NEG)
            f1 = f1 - e_ins if f1 > REACH else NEG
            f2 = f2 - (o_ins + e_ins) if f2 > REACH else NEG
            iv = max(f1, f2)
            ci = (C.get(("I", i, j - 1), 0) if f1 == iv else 0) + (C.get(("M", i, j - 1), 0) if f2 == iv else 0) if iv > REACH else 0
            M[(i, j)], D[(i, j)], I[(i, j)] = mv, dv, iv
            C[("M", i, j)], C[("D", i, j)], C[("I", i, j)] = cm, cd, ci
            h = max(mv, dv, iv)
            H[(i, j)] = h
            C[("H", i, j)] = (cm if mv == h else 0) + (cd if dv == h else 0) + (ci if iv == h else 0) if h > REACH else 0
            for v in (mv, dv, iv):
                see(v)
            if mv > REACH:
                see(mv - (o_del + e_del)); see(mv - (o_ins + e_ins))
    return dict(M=M, D=D, I=I, H=H, score=H.get((n, m), NEG), n_paths=C.get(("H", n, m), 0), lo=lo, hi=hi)


def backtrace(opt, mats, n, m):
    """SECOND RESTATEMENT of the preference among tied paths: from the last cell, M before D before I; a gap that opens or extends at equal score opens.  Returns
    (op, length) pairs, 0 = M, 1 = I, 2 = D."""
    _, _, o_del, e_del, o_ins, e_ins = scores_of(opt)
    M, D, I, H = mats["M"], mats["D"], mats["I"], mats["H"]
    ops, i, j, st = [], n, m, "H"
    met = mats.setdefault("ties_met", dict(h=0, h3=0, oe=0))        # on the path taken: cells where two / all three states tie, gaps that could open or extend
    while i > 0 and j > 0:
        if st == "H":
            h = H[(i, j)]
            k = (M[(i, j)] == h) + (D[(i, j)] == h) + (I[(i, j)] == h)
            met["h"] += k > 1; met["h3"] += k == 3
            st = "M" if M[(i, j)] == h else "D" if D[(i, j)] == h else "I"
        if st == "M":
            ops.append(0); i -= 1; j -= 1; st = "H"
        elif st == "D":
            ext = D.get((i - 1, j), NEG)
            ext = ext - e_del if ext > REACH else NEG
            opn = M.get((i - 1, j), NEG)
            opn = opn - (o_del + e_del) if opn > REACH else NEG
            ops.append(2); i -= 1
            met["oe"] += ext == opn and ext > REACH
            st = "D" if ext > opn else "M"
        else:
            ext = I.get((i, j - 1), NEG)
            ext = ext - e_ins if ext > REACH else NEG
            opn = M.get((i, j - 1), NEG)
            opn = opn - (o_ins + e_ins) if opn > REACH else NEG
            ops.append(1); j -= 1
            met["oe"] += ext == opn and ext > REACH
            st = "I" if ext > opn else "M"
    ops += [2] * i + [1] * j
    ops.reverse()
    out = []
    for op in ops:
        if out and out[-1][0] == op:
            out[-1][1] += 1
        else:
            out.append([op, 1])
    return [(op, ln) for op, ln in out]


def check_cigar(opt, cigar, qa, ta, band, score):
    """DEFINITION.  What every CIGAR of the final band must be, whatever path it took."""
    assert all(ln > 0 for _, ln in cigar) and all(x[0] != y[0] for x, y in zip(cigar, cigar[1:])), cigar
    sc, qn, tn, off = dp.rescore(cigar, qa, ta, scores_of(opt))
    assert (qn, tn) == (len(qa), len(ta)) and off <= band and sc == score, (cigar, sc, score, qn, tn, off, band)


def leftmost_single_gap(opt, cigar, qa, ta):
    """DEFINITION.  For a CIGAR x M, one gap, y M: the smallest x at which the same gap earns the same score; None when the CIGAR has another shape."""
    if len(cigar) != 3 or cigar[0][0] != 0 or cigar[2][0] != 0 or cigar[1][0] not in (1, 2):
        return None
    op, g = cigar[1]
    tot = cigar[0][1] + cigar[2][1]
    want = dp.rescore(cigar, qa, ta, scores_of(opt))[0]
    for x in range(1, tot):
        if dp.rescore([(0, x), (op, g), (0, tot - x)], qa, ta, scores_of(opt))[0] == want:
            return x
    return None


def nm_md(cigar, qa, ta):
    """DEFINITION.  NM and MD of a CIGAR (before the squeeze) over the forward-strand sequences."""
    x = y = u = nm = 0
    md = ""
    for k, (op, ln) in enumerate(cigar):
        if op == 0:
            for i in range(ln):
                if qa[x + i] != ta[y + i] or qa[x + i] > 3:
                    md += "%d%s" % (u, "ACGTN"[ta[y + i]]); u = 0; nm += 1
                else:
                    u += 1
            x += ln; y += ln
        elif op == 2:
            if 0 < k < len(cigar) - 1:
                md += "%d^%s" % (u, "".join("ACGTN"[c] for c in ta[y:y + ln])); u = 0; nm += ln
            y += ln
        else:
            x += ln; nm += ln
    return nm, md + "%d" % u


def rebuild(cigar, md, fwd_read):
    """the reference text a record implies: the read (forward-strand orientation, clips included) under the final CIGAR with MD's letters put in"""
    items, k = [], 0
    while k < len(md):                     # MD -> a list of match runs, single mismatch letters and ^deletions
        if md[k].isdigit():
            e = k
            while e < len(md) and md[e].isdigit():
                e += 1
            items.append(int(md[k:e])); k = e
        elif md[k] == "^":
            e = k + 1
            while e < len(md) and md[e].isalpha():
                e += 1
            items.append("^" + md[k + 1:e]); k = e
        else:
            items.append(md[k]); k += 1
    out, x = [], 0
    it = iter(items)
    run = 0

    def take_match(n):                     # n aligned columns: from the read, MD's letters where it names them
        nonlocal run, x
        while n > 0:
            if run == 0:
                nxt = next(it)
                if isinstance(nxt, int):
                    run = nxt
                    continue
                assert not nxt.startswith("^"), (md, cigar)
                out.append("ACGTN".index(nxt)); x += 1; n -= 1
                continue
            s = min(run, n)
            out.extend(fwd_read[x:x + s]); x += s; n -= s; run -= s
    for op, ln in cigar:
        if op == 0:
            take_match(ln)
        elif op in (1, 3):
            x += ln
        elif op == 2:
            assert run == 0, (md, cigar)
            nxt = next(it)
            if isinstance(nxt, int):
                assert nxt == 0, (md, cigar)
                nxt = next(it)
            assert nxt.startswith("^") and len(nxt) == ln + 1, (md, cigar, nxt)
            out.extend("ACGTN".index(c) for c in nxt[1:])
    return out


def record(opt, ref, read, reg, rq):
    """the record of request rq (dict: read is implied; reg None for the unmapped record; kind, owner, flag, mapq) on region reg (dict of the region's fields) of
    `read' (codes).  Returns a dict over FIELDS plus what the tests assert about the way there: rounds, band, n_paths, forced, leftmost, raw_n_cigar, n_col_rows,
    lo / hi (final band), lo_first / hi_first, gap_free."""
    if reg is None:
        return dict(pos=-1, rid=-1, flag=rq["flag"] | 4, mapq=0, NM=0, score=0, sub=0, n_cigar=0, is_rev=0, l_md=0, reg_idx=-1, xa_cnt=0, kind=None, cigar=[], md="")
    L = ref.l_pac
    rb, re, qb, qe = reg["rb"], reg["re"], reg["qb"], reg["qe"]
    assert 0 <= rb < re <= 2 * L and not rb < L < re and 0 <= qb < qe <= len(read)
    is_rev = rb >= L
    if is_rev:
        f0, f1 = 2 * L - re, 2 * L - rb
        qa = [4 if c > 3 else 3 - c for c in reversed(read[qb:qe])]
        fwd_read = [4 if c > 3 else 3 - c for c in reversed(read)]
    else:
        f0, f1 = rb, re
        qa = list(read[qb:qe])
        fwd_read = list(read)
    ta = [ref.base(p) for p in range(f0, f1)]
    rs = rounds(opt, qa, ta, w2_of(opt, len(qa), len(ta), reg["truesc"], reg["w"]), reg["truesc"])
    w2, band, score = rs[-1]
    info = dict(rounds=rs, band=band, gap_free=band is None, lo=0, hi=0, lo_first=0, hi_first=0, n_paths=1, leftmost=None, n_col_rows=0, ties_met=dict(h=0, h3=0, oe=0))
    if band is None:
        cigar = [(0, len(qa))]
    else:
        mats = band_dp(opt, qa, ta, band)
        assert mats["score"] == score, (mats["score"], score)          # the two statements of the optimum agree
        cigar = backtrace(opt, mats, len(ta), len(qa))
        check_cigar(opt, cigar, qa, ta, band, score)
        info.update(lo=mats["lo"], hi=mats["hi"], n_paths=mats["n_paths"], ties_met=mats["ties_met"], n_col_rows=min(len(qa), 2 * band + 1) * len(ta))
        first = mats if rs[0][1] == band else band_dp(opt, qa, ta, rs[0][1])
        info.update(lo_first=first["lo"], hi_first=first["hi"])
        lm = leftmost_single_gap(opt, cigar, qa, ta)
        if lm is not None:
            assert lm == cigar[0][1], ("a single gap is not at its leftmost place", cigar, lm)
            info["leftmost"] = lm
    info["forced"] = info["n_paths"] == 1
    info["raw_n_cigar"] = len(cigar)
    nm, md = nm_md(cigar, qa, ta)
    pos = f0
    if cigar[0][0] == 2:
        pos += cigar[0][1]; cigar = cigar[1:]
    elif cigar[-1][0] == 2:
        cigar = cigar[:-1]
    left, right = (len(read) - qe, qb) if is_rev else (qb, len(read) - qe)
    cigar = ([(3, left)] if left else []) + cigar + ([(3, right)] if right else [])
    if cigar and 0 <= pos < L:
        # (a trailing deletion that stays because a leading one was removed has no letters in MD: the text is rebuilt up to it)
        walk = [c for c in cigar if c[0] != 3]
        walk = cigar if walk[-1][0] != 2 else [c for c in cigar[:len(cigar) - (2 if right else 1)]]
        span = sum(ln for op, ln in walk if op in (0, 2))
        assert rebuild(walk, md, fwd_read) == [ref.base(p) for p in range(pos, pos + span)], ("read + CIGAR + MD do not give back the reference", cigar, md)
    rid = ref.rid_of(pos)
    out = dict(pos=pos - ref.ctg_off[rid], rid=rid, flag=rq["flag"] | (0x100 if reg["secondary"] >= 0 else 0), mapq=rq["mapq"], NM=nm, score=reg["score"],
               sub=max(reg["sub"], reg["csub"]), n_cigar=len(cigar), is_rev=int(is_rev), l_md=len(md), reg_idx=rq["owner"], xa_cnt=0, kind=rq["kind"],
               cigar=[ln << 4 | op for op, ln in cigar], md=md)
    out.update(info)
    return out
