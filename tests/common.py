"""Shared test helpers: seeded inputs and the comparison routines used by both the CPU-side tests
(host-emulation build of the kernel sources) and the `-m gpu` parity tests (HIP build)."""
import os
import time

import numpy as np

import simreads
from speedseq_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXAMPLE_FA = os.path.join(GOLDEN, "chr20_slice.fa")

KSW_XBYTE, KSW_XSTOP, KSW_XSUBO, KSW_XSTART = 0x10000, 0x20000, 0x40000, 0x80000


def mutate(rng, q, max_sub=8, max_indel=3):
    tl = list(q)
    for _ in range(int(rng.integers(0, max_sub))):
        if not tl:
            break
        p = int(rng.integers(0, len(tl)))
        tl[p] = (tl[p] + 1) % 4
    for _ in range(int(rng.integers(0, max_indel))):
        if len(tl) < 2:
            break
        p = int(rng.integers(0, len(tl)))
        if rng.random() < 0.5:
            del tl[p:p + int(rng.integers(1, 8))]
        else:
            tl[p:p] = list(rng.integers(0, 4, size=int(rng.integers(1, 8))))
    return tl


def scored_opts(lib, oracle, scores):
    """(option block of the library, option block of the oracle or None) with scores = (a, b, o_del, e_del, o_ins, e_ins); None: the defaults"""
    opt = lib.opt_init() if lib is not None else None
    if not scores:
        return opt, None
    if opt is not None:
        for k, v in zip(("a", "b", "o_del", "e_del", "o_ins", "e_ins"), scores):
            opt[k] = v
        m = opt["mat"][0]
        for x in range(4):
            for y in range(4):
                m[x * 5 + y] = scores[0] if x == y else -scores[1]
    return opt, (oracle.opt_scores(*scores) if oracle is not None else None)


def make_extend_jobs(n, seed, max_qlen=200, scores=None, end_bonus=5):
    """scores: the anchor's score h0 is drawn in matches (1 .. 159 times a), as upstream's seeds give it"""
    rng = np.random.default_rng(seed)
    jobs, qs, ts, qo, to = [], [], [], 0, 0
    for _ in range(n):
        qlen = int(rng.integers(1, max_qlen))
        q = rng.integers(0, 4, size=qlen, dtype=np.uint8)
        mode = rng.integers(0, 4)
        tl = list(q)
        if mode >= 1:
            tl = mutate(rng, q, 6, 1)
        if mode >= 2:
            tl = mutate(rng, np.array(tl, dtype=np.uint8), 3, 3)
        if mode == 3 and len(tl) > 10:
            tl = tl[:int(len(tl) * rng.random()) + 1] + list(rng.integers(0, 4, size=30))
        tl += list(rng.integers(0, 4, size=int(rng.integers(0, 120))))
        t = np.array(tl, dtype=np.uint8)
        if rng.random() < 0.1:
            q[rng.integers(0, qlen)] = 4
        h0 = int(rng.integers(1, 160))
        w = int(rng.choice([100, 200, 5, 20]))
        zd = int(rng.choice([100, 100, 0, 20]))
        jobs.append((qo, qlen, to, len(t), w, end_bonus, zd, h0 * (scores[0] if scores else 1)))
        qs.append(q)
        ts.append(t)
        qo += qlen
        to += len(t)
    return np.array(jobs, dtype=capi.EXT_JOB_DT), qs, ts


def local_xtra(qlen, scores=None):
    """xtra as mate rescue sets it: 8-bit cells where the best possible score stays under 250, the seed's score as the threshold"""
    a = scores[0] if scores else 1
    return KSW_XSUBO | KSW_XSTART | (KSW_XBYTE if qlen * a < 250 else 0) | (19 * a)


def make_local_jobs(n, seed, qlens=(150, 150, 100, 76, 36, 250, 200), scores=None):
    rng = np.random.default_rng(seed)
    jobs, qs, ts, qo, to = [], [], [], 0, 0
    for _ in range(n):
        qlen = int(rng.choice(list(qlens)))
        q = rng.integers(0, 4, size=qlen, dtype=np.uint8)
        mid = mutate(rng, q) if rng.random() < 0.8 else list(rng.integers(0, 4, size=50))
        if rng.random() < 0.3:
            mid = mid[:len(mid) // 2]
        t = np.array(list(rng.integers(0, 4, size=int(rng.integers(0, 300)))) + mid +
                     list(rng.integers(0, 4, size=int(rng.integers(0, 300)))), dtype=np.uint8)
        if rng.random() < 0.3:
            t = np.concatenate([t, np.array(mutate(rng, q), dtype=np.uint8)])
        xtra = local_xtra(qlen, scores)
        jobs.append((qo, qlen, to, len(t), xtra, 0))
        qs.append(q)
        ts.append(t)
        qo += qlen
        to += len(t)
    return np.array(jobs, dtype=capi.SW_JOB_DT), qs, ts


def make_global_jobs(n, seed, scores=None):
    """scores: accepted like the other generators'; a global job carries no field that scales with the scoring, so the jobs do not depend on it"""
    rng = np.random.default_rng(seed)
    jobs, qs, ts, qo, to = [], [], [], 0, 0
    for _ in range(n):
        qlen = int(rng.integers(5, 250))
        q = rng.integers(0, 4, size=qlen, dtype=np.uint8)
        t = np.array(mutate(rng, q), dtype=np.uint8)
        w = abs(len(t) - qlen) + int(rng.integers(3, 40))
        jobs.append((qo, qlen, to, len(t), w, 0))
        qs.append(q)
        ts.append(t)
        qo += qlen
        to += len(t)
    return np.array(jobs, dtype=capi.GLB_JOB_DT), qs, ts


def sim_reads(n_pairs, seed, read_len=150, fasta=EXAMPLE_FA, **kw):
    contigs = simreads.read_fasta(fasta)
    pairs = simreads.simulate(contigs, n_pairs, seed=seed, read_len=read_len, **kw)
    seqs = []
    for _, r1, r2 in pairs:
        seqs += [r1, r2]
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return pairs, seqs, np.concatenate(seqs), off



COLUMN_CLASSES = (40, 72, 136, 256, 320)


def _edge_qlens(max_qlen, extra=()):
    """1, 2, either side of every column class, and the longest query the entry point takes with the one before it"""
    ls = {1, 2, max_qlen - 1, max_qlen}
    for cap in COLUMN_CLASSES:
        ls.update((cap - 1, cap, cap + 1))
    ls.update(extra)
    return sorted(l for l in ls if 1 <= l <= max_qlen)


def fixed_extend_shapes(seed, max_qlen, scores=None):
    """The shapes a random draw only meets by chance, as (q, t, w, zdrop, h0 in matches): query lengths 1, 2 and either side of every column
    class, a target of one base, an all-N query, a target that matches nowhere (the first row dies), h0 = 1, a target shorter than the
    band, a target longer than qlen + w."""
    rng = np.random.default_rng(seed)
    out = []
    for ql in _edge_qlens(max_qlen):
        q = rng.integers(0, 4, size=ql, dtype=np.uint8)
        t = np.array(mutate(rng, q, 4, 2) + list(rng.integers(0, 4, size=int(rng.integers(0, 30)))), dtype=np.uint8)
        if t.size == 0:
            t = q.copy()
        out.append((q, t, int(rng.choice([100, 20])), 100, int(rng.integers(1, 40))))
    ql = min(60, max_qlen)
    q = rng.integers(0, 4, size=ql, dtype=np.uint8)
    out.append((q, q[:1].copy(), 100, 100, 30))                                           # tlen 1
    out.append((np.full(ql, 4, dtype=np.uint8), rng.integers(0, 4, size=ql + 10, dtype=np.uint8), 100, 100, 25))   # all N
    out.append((np.zeros(ql, dtype=np.uint8), np.full(ql + 5, 1, dtype=np.uint8), 100, 100, 1))    # no base matches: the first row is dead
    out.append((q, np.concatenate([q, q[:20]]), 100, 0, 1))                               # h0 == 1 on a perfect target: a live cell at the lowest score
    out.append((q, q[:7].copy(), 20, 100, 40))                                            # target shorter than the band
    out.append((q, np.concatenate([q, rng.integers(0, 4, size=5 + 40, dtype=np.uint8)]), 5, 0, 40))   # target longer than qlen + w, no z-drop
    return out


def add_extend_shapes(jobs, qs, ts, shapes, scores=None, end_bonus=5):
    a = scores[0] if scores else 1
    qs, ts, rows = list(qs), list(ts), [tuple(j) for j in jobs]
    qo, to = sum(len(q) for q in qs), sum(len(t) for t in ts)
    for q, t, w, zd, h0 in shapes:
        rows.append((qo, len(q), to, len(t), w, end_bonus, zd, h0 * a if h0 > 1 else 1))
        qs.append(q); ts.append(t)
        qo += len(q); to += len(t)
    return np.array(rows, dtype=capi.EXT_JOB_DT), qs, ts


def fixed_local_shapes(seed, max_qlen=320, scores=None):
    """(q, t) for the local alignment: query lengths 1, 2, either side of every column class, 249 / 250 and the last length with 8-bit cells at this match
    score with the first one with 16-bit cells (249 // a, 249 // a + 1: where local_xtra switches KSW_XBYTE), 257 and 320; a target of one base; an all-N
    query; a target that matches nowhere"""
    rng = np.random.default_rng(seed)
    out = []
    a = scores[0] if scores else 1
    for ql in _edge_qlens(max_qlen, (249, 250, 257, 320, 249 // a, 249 // a + 1)):
        q = rng.integers(0, 4, size=ql, dtype=np.uint8)
        t = np.array(list(rng.integers(0, 4, size=int(rng.integers(0, 60)))) + mutate(rng, q, 5, 2) + list(rng.integers(0, 4, size=int(rng.integers(1, 60)))), dtype=np.uint8)
        out.append((q, t))
    q = rng.integers(0, 4, size=50, dtype=np.uint8)
    out.append((q, q[10:11].copy()))
    out.append((np.full(50, 4, dtype=np.uint8), rng.integers(0, 4, size=80, dtype=np.uint8)))
    out.append((np.zeros(50, dtype=np.uint8), np.full(70, 1, dtype=np.uint8)))
    return out


def add_local_shapes(jobs, qs, ts, shapes, scores=None):
    qs, ts, rows = list(qs), list(ts), [tuple(j) for j in jobs]
    qo, to = sum(len(q) for q in qs), sum(len(t) for t in ts)
    for q, t in shapes:
        rows.append((qo, len(q), to, len(t), local_xtra(len(q), scores), 0))
        qs.append(q); ts.append(t)
        qo += len(q); to += len(t)
    return np.array(rows, dtype=capi.SW_JOB_DT), qs, ts


def fixed_global_shapes(seed, max_qlen=318):
    """(q, t, w) for the global alignment: w == |tlen - qlen| (the band's corner is the last cell), w larger than both lengths, qlen 1, tlen 1, query lengths
    either side of every column class, an all-N query, a target that matches nowhere"""
    rng = np.random.default_rng(seed)
    out = []
    for ql in _edge_qlens(max_qlen):
        q = rng.integers(0, 4, size=ql, dtype=np.uint8)
        t = np.array(mutate(rng, q, 5, 3), dtype=np.uint8)
        if t.size == 0:
            t = q.copy()
        out.append((q, t, abs(len(t) - ql) + int(rng.integers(0, 12))))
    for _ in range(4):                                                                   # w == |tlen - qlen|, the lengths different
        q = rng.integers(0, 4, size=int(rng.integers(20, 120)), dtype=np.uint8)
        t = np.array(mutate(rng, q, 5, 3), dtype=np.uint8)
        if len(t) == len(q):
            t = np.concatenate([t[:10], t[13:]])
        out.append((q, t, abs(len(t) - len(q))))
    q = rng.integers(0, 4, size=30, dtype=np.uint8)
    out.append((q, q.copy(), 0))                                                         # equal lengths, w == 0: the diagonal alone
    out.append((q, np.array(mutate(rng, q, 4, 2), dtype=np.uint8), 100))                 # w larger than both lengths
    out.append((q[:1].copy(), q[:9].copy(), 8))                                          # qlen 1
    out.append((q[:9].copy(), q[3:4].copy(), 8))                                         # tlen 1
    out.append((q[:1].copy(), q[:1].copy(), 3))
    out.append((np.full(30, 4, dtype=np.uint8), q[:27].copy(), 6))
    out.append((np.zeros(30, dtype=np.uint8), np.full(33, 1, dtype=np.uint8), 5))
    return out


def add_global_shapes(jobs, qs, ts, shapes):
    qs, ts, rows = list(qs), list(ts), [tuple(j) for j in jobs]
    qo, to = sum(len(q) for q in qs), sum(len(t) for t in ts)
    for q, t, w in shapes:
        rows.append((qo, len(q), to, len(t), w, 0))
        qs.append(q); ts.append(t)
        qo += len(q); to += len(t)
    return np.array(rows, dtype=capi.GLB_JOB_DT), qs, ts


class RefTally:
    """what a run compared with the full-matrix reference: jobs, and the jobs whose gtle the `gscore <= 0' rule left out"""
    def __init__(self):
        self.jobs = self.ext_jobs = self.gtle_excluded = 0
        self.seconds = 0.0   # spent inside tests/dp_reference.py: what the tests' job counts are sized by

    def check_share(self):
        """under one in ten of the extension jobs"""
        assert self.jobs > 0 and self.ext_jobs > 0 and 10 * self.gtle_excluded < self.ext_jobs, "gtle left uncompared on %d of %d extensions" % (self.gtle_excluded, self.ext_jobs)


DEFAULT_SCORES = (1, 4, 6, 1, 6, 1)


def ref_check_extend(got, q, t, scores, w, end_bonus, zdrop, h0, tally, who, ctx):
    """got = (score, qle, tle, gtle, gscore, max_off) against tests/dp_reference.py: score, qle, tle, max_off equal; gscore equal or both <= 0; gtle equal
    where gscore > 0"""
    import dp_reference
    t0 = time.perf_counter()
    r = dp_reference.extend(q, t, scores or DEFAULT_SCORES, w, end_bonus, zdrop, h0)
    tally.seconds += time.perf_counter() - t0
    msg = ("%s disagrees with the full-matrix reference" % who, ctx, "got", got, "reference", r)
    assert (got[0], got[1], got[2], got[5]) == (r[0], r[1], r[2], r[5]), msg
    assert got[4] == r[4] or (got[4] <= 0 and r[4] <= 0), msg
    if r[4] > 0:
        assert got[3] == r[3], msg
    elif got[3] != r[3]:
        tally.gtle_excluded += 1
    tally.jobs += 1
    tally.ext_jobs += 1


def ref_check_local(got, q, t, xtra, scores, tally, who, ctx):
    """got = (score, te, qe, score2, te2, tb, qb): score is the maximum of the reference's H, H[te][qe] holds it, and where a start is reported the global
    alignment of q[qb..qe] and t[tb..te] earns the same.  score2 / te2 are not the reference's business."""
    import dp_reference
    sc = scores or DEFAULT_SCORES
    t0 = time.perf_counter()
    H = dp_reference.local(q, t, sc)
    tally.seconds += time.perf_counter() - t0
    score, te, qe, tb, qb = got[0], got[1], got[2], got[5], got[6]
    msg = ("%s disagrees with the full-matrix reference" % who, ctx, "got", got, "reference maximum", int(H.max()))
    assert score == int(H.max()), msg
    assert -1 <= te < len(t) and -1 <= qe < len(q) and int(H[te + 1][qe + 1]) == score, msg
    if (xtra & KSW_XSTART) and not ((xtra & KSW_XSUBO) and score < (xtra & 0xffff)):
        assert 0 <= tb <= te and 0 <= qb <= qe, msg
        g = dp_reference.global_(q[qb:qe + 1], t[tb:te + 1], sc, len(q) + len(t))
        assert g == score, msg + ("global score of the reported substrings", g)
    tally.jobs += 1


def ref_check_global(score, n_cigar, cigar, q, t, w, scores, tally, who, ctx):
    """the score is the reference's banded optimum; the CIGAR consumes both sequences whole, stays in the band and earns that score"""
    import dp_reference
    sc = scores or DEFAULT_SCORES
    t0 = time.perf_counter()
    r = dp_reference.global_(q, t, sc, w)
    tally.seconds += time.perf_counter() - t0
    msg = ("%s disagrees with the full-matrix reference" % who, ctx, "got", int(score), "reference", r)
    assert int(score) == r, msg
    assert 0 < n_cigar <= len(cigar), msg
    rs, qn, tn, off = dp_reference.rescore(cigar[:n_cigar], q, t, sc)
    assert (qn, tn) == (len(q), len(t)) and off <= w and rs == r, msg + ("cigar", [(int(c) & 0xf, int(c) >> 4) for c in cigar[:n_cigar]], "earns", rs, "consumes", qn, tn, "leaves the diagonal by", off)
    tally.jobs += 1


REG_FIELDS = ["rb", "re", "qb", "qe", "rid", "score", "truesc", "sub", "csub", "w", "seedcov", "seedlen0", "n_comp", "frac_rep"]


def check_extend(lib, oracle, n, seed, max_qlen=200, scores=None, end_bonus=5, ref=None, fixed=False):
    """ref: a RefTally -- every job is compared with tests/dp_reference.py too; fixed: the shapes of fixed_extend_shapes follow the random jobs"""
    jobs, qs, ts = make_extend_jobs(n, seed, max_qlen=max_qlen, scores=scores, end_bonus=end_bonus)
    if fixed:
        jobs, qs, ts = add_extend_shapes(jobs, qs, ts, fixed_extend_shapes(seed, max_qlen, scores), scores, end_bonus)
    opt, oopt = scored_opts(lib, oracle, scores)
    res, cells = lib.extend_batch(opt, jobs, np.concatenate(qs), np.concatenate(ts))
    for i in range(len(jobs)):
        o = oracle.extend2(qs[i], ts[i], int(jobs[i]["w"]), end_bonus, int(jobs[i]["zdrop"]), int(jobs[i]["h0"]), oopt)
        got = tuple(int(x) for x in res[i])
        assert o == got, ("extend_batch disagrees with the oracle", scores, i, jobs[i], o, res[i])
        if ref is not None:
            ref_check_extend(got, qs[i], ts[i], scores, int(jobs[i]["w"]), end_bonus, int(jobs[i]["zdrop"]), int(jobs[i]["h0"]), ref, "extend_batch", (scores, i, jobs[i]))
    assert cells > 0


def check_extend_lane(lib, oracle, n, seed, workdir, qcaps=(72, 136, 256), scores=None, end_bonus=5, ref=None, fixed=False):
    """ksw_extend2 through the lane-per-extension kernel code of the product's mem_chain2aln path (ssg_k_ext_lane's ln_extend2: packed 13-bit
    cells in LDS, 6-bit score table, targets read from the 2-bit reference) against the oracle: the jobs of make_extend_jobs (w 5 / 20 / 100 /
    200, zdrop 0 / 20 / 100, N in the query, h0 1..160) plus h0 up to the 13-bit ceiling, their targets laid out as a reference of their
    own, read forward, backward and from the reverse strand (the four ways the product's left / right extensions walk the reference).
    scores / end_bonus: queries no longer than the 13-bit cells hold at that match score; ref / fixed: as check_extend."""
    rng = np.random.default_rng(seed)
    fa = os.path.join(str(workdir), "extlane_%d.fa" % seed)
    done = 0
    a = scores[0] if scores else 1
    opt, oopt = scored_opts(lib, oracle, scores)
    for qcap in qcaps:
        max_qlen = min(qcap, 318, (8190 - end_bonus - 1) // a)   # h0 >= 1 must still fit
        jobs, qs, ts = make_extend_jobs(n, seed + qcap, max_qlen=max_qlen + 1, scores=scores, end_bonus=end_bonus)
        for i in range(n):   # a share of the jobs with start scores near the ceiling of the packed cells (h0 + qlen * a + end_bonus < 8191)
            ceil = 8190 - int(jobs[i]["qlen"]) * a - end_bonus
            if rng.random() < 0.15:
                jobs[i]["h0"] = max(1, ceil - int(rng.integers(0, 60)))
            elif jobs[i]["h0"] > ceil:
                jobs[i]["h0"] = ceil
        if fixed:   # appended after the draw above: the fixed shapes keep their own h0, lowered only where the cells could not hold it
            jobs, qs, ts = add_extend_shapes(jobs, qs, ts, fixed_extend_shapes(seed + qcap, max_qlen, scores), scores, end_bonus)
            for i in range(len(ts)):   # the targets come from a 2-bit reference, and a job's target is not empty
                if ts[i].size == 0:
                    ts[i] = qs[i][:1].copy() if qs[i][0] < 4 else np.zeros(1, dtype=np.uint8)
            jobs["tlen"] = [t.size for t in ts]
            jobs["toff"] = np.concatenate([[0], np.cumsum([t.size for t in ts])[:-1]])
            for i in range(n, len(jobs)):
                jobs[i]["h0"] = min(int(jobs[i]["h0"]), 8190 - int(jobs[i]["qlen"]) * a - end_bonus)
        m = len(jobs)
        tcat = np.concatenate(ts)
        with open(fa, "w") as f:
            f.write(">t\n")
            txt = "".join("ACGT"[c] for c in tcat)
            for k in range(0, len(txt), 80):
                f.write(txt[k:k + 80] + "\n")
        idx = lib.index_build_fasta(fa)
        L = int(tcat.size)
        starts = jobs["toff"].astype(np.int64)
        tl = jobs["tlen"].astype(np.int64)
        comp = lambda a: (3 - a).astype(np.uint8)
        modes = [("fwd +1", starts, 1, lambda t: t), ("fwd -1", starts + tl - 1, -1, lambda t: t[::-1]),
                 ("rev +1", 2 * L - starts - tl, 1, lambda t: comp(t[::-1])), ("rev -1", 2 * L - 1 - starts, -1, lambda t: comp(t))]
        for name, tpos, d, view in modes:
            res, cells = lib.extend_lane_batch(idx, opt, jobs, tpos, d, np.concatenate(qs), qcap)
            assert cells > 0
            for i in range(m):
                tv = np.ascontiguousarray(view(ts[i]))
                o = oracle.extend2(qs[i], tv, int(jobs[i]["w"]), end_bonus, int(jobs[i]["zdrop"]), int(jobs[i]["h0"]), oopt)
                got = tuple(int(x) for x in res[i])
                assert o == got, ("extend_lane_batch disagrees with the oracle", scores, qcap, name, i, jobs[i], o, res[i])
                if ref is not None:
                    ref_check_extend(got, qs[i], tv, scores, int(jobs[i]["w"]), end_bonus, int(jobs[i]["zdrop"]), int(jobs[i]["h0"]), ref, "extend_lane_batch", (scores, qcap, name, i, jobs[i]))
            done += m
        lib.index_destroy(idx)
    return done


def check_local_lane(lib, oracle, n, seed, workdir, lanes=(1, 2, 4), scores=None, qlens=None, ref=None, fixed=False, expect_lane=True):
    """ksw_align2 as mate rescue runs it in the product path (k_mswlane.h: forward pass by the lane kernel -- strips of 8 target rows in
    registers, packed 13-bit strip boundaries in LDS, 5-bit score table, targets from the 2-bit reference --, reverse pass by the wave code)
    against the oracle: make_local_jobs' queries (36 .. 250 bases, some with N) and targets (hits, half hits, second hits, none), the targets
    laid out as a reference of their own and read from both strands, 1 / 2 / 4 lanes per job.
    ref: a RefTally -- xtra follows the scores (local_xtra) and every job is compared with tests/dp_reference.py too; fixed: the shapes of
    fixed_local_shapes follow the random jobs; expect_lane False: scoring the lane kernel must refuse -- every job through the wave form."""
    rng = np.random.default_rng(seed)
    kw = dict(scores=scores) if ref is not None else {}
    jobs, qs, ts = make_local_jobs(n, seed, qlens, **kw) if qlens else make_local_jobs(n, seed, **kw)
    if fixed:
        jobs, qs, ts = add_local_shapes(jobs, qs, ts, fixed_local_shapes(seed, scores=scores), scores)
        n = len(jobs)
    for i in range(n):
        if rng.random() < 0.2:   # N bases in the query
            q = qs[i].copy(); q[rng.random(q.size) < 0.03] = 4; qs[i] = q
        if ts[i].size == 0:
            ts[i] = rng.integers(0, 4, size=40, dtype=np.uint8)
    to = 0
    for i in range(n):
        jobs[i]["toff"] = to; jobs[i]["tlen"] = ts[i].size; to += ts[i].size
    tcat = np.concatenate(ts)
    fa = os.path.join(str(workdir), "locallane_%d.fa" % seed)
    with open(fa, "w") as f:
        f.write(">t\n")
        txt = "".join("ACGT"[c] for c in tcat)
        for k in range(0, len(txt), 80):
            f.write(txt[k:k + 80] + "\n")
    idx = lib.index_build_fasta(fa)
    L = int(tcat.size)
    starts = jobs["toff"].astype(np.int64)
    tl = jobs["tlen"].astype(np.int64)
    opt, oopt = scored_opts(lib, oracle, scores)   # (a, b, o_del, e_del, o_ins, e_ins)
    done = taken = 0
    rc = lambda a: np.where(a[::-1] < 4, 3 - a[::-1], 4).astype(np.uint8)
    for name, tpos, view, qview in (("fwd", starts, lambda t: t, lambda q: q), ("rev", 2 * L - starts - tl, rc, rc)):   # the reverse strand reads the windows reverse-complemented: so are the queries, or nothing would hit
        qv = [np.ascontiguousarray(qview(q)) for q in qs]
        tv = [np.ascontiguousarray(view(t)) for t in ts]
        want = [oracle.align2(qv[i], tv[i], int(jobs[i]["xtra"]), oopt) for i in range(n)]
        if ref is not None:   # the oracle's answer once per strand; the kernel's must equal it for every lane count below
            for i in range(n):
                ref_check_local(want[i], qv[i], tv[i], int(jobs[i]["xtra"]), scores, ref, "the oracle", (scores, name, i, jobs[i]))
        for nl in lanes:
            res, from_lane = lib.align2_lane_batch(idx, opt, jobs, tpos, np.concatenate(qv), nl)
            for i in range(n):
                assert want[i] == tuple(int(x) for x in res[i]), ("align2_lane_batch disagrees with the oracle", scores, nl, name, i, jobs[i], want[i], res[i], int(from_lane[i]))
            done += n
            taken += int((from_lane > 0).sum())
            if expect_lane:
                assert (from_lane == 2).sum() > n // 4, "the reverse passes did not go through the lane kernel"
            else:
                assert (from_lane == 0).all(), "scoring beyond the lane kernel's fields went through it"
    lib.index_destroy(idx)
    return done, taken


def check_seeds(lib, oracle, n_pairs, seed, prefix=EXAMPLE_FA, read_len=150, ref=None, ref_n=16):
    """the seeds mem_chain visits (interval -> sampled occurrences -> bwt_sa + bns_intv2rid, upstream's order) straight from ssg_k_sal against the oracle;
    ref: a SeedTally -- the first ref_n reads are compared with tests/seed_reference.py too"""
    oidx, gidx = oracle.idx_load(prefix), lib.index_load(prefix)
    _, seqs, seq, off = sim_reads(n_pairs, seed, read_len, fasta=prefix)
    seed_off, seeds, rids = lib.seeds_batch(gidx, lib.opt_init(), seq, off)
    tot = 0
    for r, s in enumerate(seqs):
        o = oracle.seeds(oidx, s)
        g = seeds[seed_off[r]:seed_off[r + 1]]
        assert len(o) == len(g), (r, len(o), len(g))
        assert np.array_equal(o[:, 0], g["rbeg"]) and np.array_equal(o[:, 1], g["qbeg"]) and np.array_equal(o[:, 2], g["len"]), r
        assert np.array_equal(o[:, 3], rids[seed_off[r]:seed_off[r + 1]]), r
        if ref is not None and r < ref_n:
            ref_check_seeds(g, rids[seed_off[r]:seed_off[r + 1]], s, None, seed_ref(prefix), ref, "seeds_batch", (prefix, seed, r))
        tot += len(o)
    if ref is not None:
        ref.check()
    lib.index_destroy(gidx)
    return tot


def check_local(lib, oracle, n, seed, scores=None, ref=None, fixed=False):
    """ref / fixed: as check_local_lane"""
    jobs, qs, ts = make_local_jobs(n, seed, scores=scores)
    if fixed:
        jobs, qs, ts = add_local_shapes(jobs, qs, ts, fixed_local_shapes(seed, scores=scores), scores)
    opt, oopt = scored_opts(lib, oracle, scores)
    res = lib.align2_batch(opt, jobs, np.concatenate(qs), np.concatenate(ts))
    for i in range(len(jobs)):
        o = oracle.align2(qs[i], ts[i], int(jobs[i]["xtra"]), oopt)
        got = tuple(int(x) for x in res[i])
        assert o == got, ("align2_batch disagrees with the oracle", scores, i, jobs[i], o, res[i])
        if ref is not None:
            ref_check_local(got, qs[i], ts[i], int(jobs[i]["xtra"]), scores, ref, "align2_batch", (scores, i, jobs[i]))


def check_global(lib, oracle, n, seed, scores=None, ref=None, fixed=False):
    """ref: a RefTally -- score and CIGAR are checked against tests/dp_reference.py too (the CIGAR buffers are then long enough for every path); fixed: the
    shapes of fixed_global_shapes follow the random jobs"""
    jobs, qs, ts = make_global_jobs(n, seed, scores=scores)
    if fixed:
        jobs, qs, ts = add_global_shapes(jobs, qs, ts, fixed_global_shapes(seed))
    opt, oopt = scored_opts(lib, oracle, scores)
    cap = 64 if ref is None else 1024
    sc, nc, cg = lib.global_batch(opt, jobs, np.concatenate(qs), np.concatenate(ts), cap=cap)
    for i in range(len(jobs)):
        osc, on, ocg = oracle.global2(qs[i], ts[i], int(jobs[i]["w"]), cap=cap, opt=oopt)
        assert osc == sc[i] and on == nc[i] and np.array_equal(ocg[:on], cg[i, :on]), ("global_batch disagrees with the oracle", scores, i, jobs[i])
        if ref is not None:
            ref_check_global(sc[i], int(nc[i]), cg[i], qs[i], ts[i], int(jobs[i]["w"]), scores, ref, "global_batch", (scores, i, jobs[i]))


def check_smem(lib, oracle, n_pairs, seed, read_len=150, prefix=EXAMPLE_FA, n_frac=0.0, cap=96, ref=None, ref_n=16):
    """seeding intervals (upstream mem_collect_intv) of every read against the oracle; n_frac: share of the bases turned into N;
    ref: a SeedTally -- the first ref_n reads are compared with tests/seed_reference.py too"""
    oidx, gidx = oracle.idx_load(prefix), lib.index_load(prefix)
    _, seqs, seq, off = sim_reads(n_pairs, seed, read_len, fasta=prefix)
    if n_frac > 0:
        rng = np.random.RandomState(seed)
        seq = seq.copy()
        seq[rng.random_sample(seq.size) < n_frac] = 4
        seqs = [seq[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    intv, cnt = lib.smem_batch(gidx, lib.opt_init(), seq, off, cap=cap)
    for r, s in enumerate(seqs):
        o = oracle.collect_intv(oidx, s)
        assert len(o) == cnt[r] and np.array_equal(o, intv[r, :cnt[r]]), r
        if ref is not None and r < ref_n:
            ref_check_smem(intv[r, :cnt[r]], s, None, seed_ref(prefix), ref, "smem_batch", (prefix, seed, r))
    if ref is not None:
        ref.check()
    lib.index_destroy(gidx)


def check_pe_sam(lib, oracle, n_pairs, seed, read_len=150, n_threads=8, prefix=EXAMPLE_FA, **kw):
    """Whole `bwa mem` PE hot path: SAM text from the device records must equal the oracle's."""
    oidx, gidx = oracle.idx_load(prefix), lib.index_load(prefix)
    pairs, seqs, seq, off = sim_reads(n_pairs, seed, read_len, fasta=prefix, **kw)
    names = []
    for nm, _, _ in pairs:
        names += [nm, nm]
    quals = ["I" * len(s) for s in seqs]
    opt = lib.opt_init()
    res = capi.mem_process_pairs(lib, gidx, opt, seq, off, id0=0)
    text, _ = capi.sam_format(lib, gidx, opt, res, names, seq, off, quals, "grp1")
    otext, _, opes = oracle.process_pairs(oidx, seq, off, names, quals, 0, "grp1", n_threads)
    for f in ("low", "high", "failed", "avg", "std"):
        assert np.array_equal(res.pes[f][:4], opes[f]), (f, res.pes, opes)
    if text != otext:
        a, b = text.split("\n"), otext.split("\n")
        assert len(a) == len(b), (len(a), len(b))
        for x, y in zip(a, b):
            assert x == y, "\n%s\n%s" % (x, y)
    stats = res.stats.copy()
    res.close()
    lib.index_destroy(gidx)
    return text, stats


def check_pe_edge_cases(lib, oracle):
    """Ragged / degenerate inputs the reference's aligner meets in practice: reads of different lengths,
    a read below min_seed_len, all-N reads, a random (unmappable) mate, exact duplicates, a pair count of 1."""
    prefix = EXAMPLE_FA
    oidx, gidx = oracle.idx_load(prefix), lib.index_load(prefix)
    contigs = simreads.read_fasta(prefix)
    ref = contigs[0][1]
    rng = np.random.default_rng(77)
    comp = np.array([3, 2, 1, 0, 4], dtype=np.uint8)

    def frag(pos, l):
        return ref[pos:pos + l].copy()

    def rc(s):
        return comp[s[::-1]]

    pairs = []
    pairs.append((frag(1000, 150), rc(frag(1300, 150))))                       # plain proper pair
    pairs.append((frag(1000, 150), rc(frag(1300, 150))))                       # exact duplicate of it
    pairs.append((frag(5000, 100), rc(frag(5250, 76))))                        # ragged lengths
    pairs.append((frag(9000, 12), rc(frag(9300, 150))))                        # read shorter than min_seed_len
    pairs.append((np.full(150, 4, dtype=np.uint8), rc(frag(12000, 150))))      # all-N read 1
    pairs.append((np.full(80, 4, dtype=np.uint8), np.full(80, 4, dtype=np.uint8)))  # both all-N
    pairs.append((frag(20000, 150), rng.integers(0, 4, size=150, dtype=np.uint8)))  # random mate -> rescue attempt
    pairs.append((rng.integers(0, 4, size=150, dtype=np.uint8), rng.integers(0, 4, size=150, dtype=np.uint8)))  # both random
    a = frag(30000, 150)
    a[75] = 4
    pairs.append((a, rc(frag(30310, 150))))                                    # N in the middle
    pairs.append((np.concatenate([frag(40000, 80), frag(90000, 70)]), rc(frag(40300, 150))))  # chimeric read 1
    for k in range(40):                                                         # enough proper pairs for the insert-size model
        p = 50000 + 997 * k
        pairs.append((frag(p, 150), rc(frag(p + 250 + (k % 7) * 10, 150))))
    seqs = []
    for r1, r2 in pairs:
        seqs += [r1, r2]
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    seq = np.concatenate(seqs)
    names = []
    for i in range(len(pairs)):
        names += ["e%d" % i, "e%d" % i]
    quals = ["5" * len(s) for s in seqs]
    opt = lib.opt_init()
    res = capi.mem_process_pairs(lib, gidx, opt, seq, off, id0=7)
    text, _ = capi.sam_format(lib, gidx, opt, res, names, seq, off, quals, "g")
    otext, _, _ = oracle.process_pairs(oidx, seq, off, names, quals, 14, "g", 2)
    assert text == otext, "\n".join(x + "\n" + y for x, y in zip(text.split("\n"), otext.split("\n")) if x != y)
    res.close()
    # a single pair: insert-size inference fails for every orientation, pairing falls back
    one_seq, one_off = np.concatenate(seqs[:2]), np.array([0, 150, 300], dtype=np.int64)
    res = capi.mem_process_pairs(lib, gidx, opt, one_seq, one_off, id0=0)
    t1, _ = capi.sam_format(lib, gidx, opt, res, names[:2], one_seq, one_off, quals[:2], "")
    o1, _, opes = oracle.process_pairs(oidx, one_seq, one_off, names[:2], quals[:2], 0, "", 1)
    assert t1 == o1 and all(int(x) == 1 for x in res.pes["failed"][:4])
    res.close()
    lib.index_destroy(gidx)
    return text


def sam_primary_ends(text, contig_names):
    """Per pair: the two primary records as samblaster sees them (capi.SBL_END_DT), from SAM text."""
    import re
    idx = {n: i for i, n in enumerate(contig_names)}
    ends, cur, name = [], {}, None

    def flush():
        if cur:
            ends.append(cur.get(0x40, (-1, 0, 0x4, 0, 0, 0)))
            ends.append(cur.get(0x80, (-1, 0, 0x4, 0, 0, 0)))

    for line in text.split("\n"):
        if not line or line[0] == "@":
            continue
        f = line.split("\t")
        if f[0] != name:
            flush()
            cur, name = {}, f[0]
        flag = int(f[1])
        if flag & 0x900:
            continue
        ops = re.findall(r"(\d+)([MIDNSH=X])", f[5])
        lclip = rclip = ralen = 0
        first = True
        for n, op in ops:
            n = int(n)
            if op in "SH":
                if first:
                    lclip += n
                rclip += n
            else:
                first = False
                rclip = 0
                if op in "MDN=X":
                    ralen += n
        seq = -1 if (flag & 4) or f[2] == "*" else idx[f[2]]
        cur[flag & 0xc0] = (seq, int(f[3]), flag, lclip, rclip if ops else 0, ralen)
    flush()
    return np.array(ends, dtype=capi.SBL_END_DT)


def oracle_dup_flags(oracle, sam_text, header):
    """Run the oracle samblaster over SAM text; returns per-pair dup flags (from read1 primaries)."""
    out = oracle.samblaster(header + sam_text)
    flags, name = [], None
    for line in out.split("\n"):
        if not line or line[0] == "@":
            continue
        f = line.split("\t")
        if f[0] != name:
            name = f[0]
            flags.append(1 if int(f[1]) & 0x400 else 0)
    return np.array(flags, dtype=np.uint8), out


def check_dedup(lib, oracle, n_pairs, seed, dup_frac=0.2):
    prefix = EXAMPLE_FA
    oidx = oracle.idx_load(prefix)
    pairs, seqs, seq, off = sim_reads(n_pairs, seed, dup_frac=dup_frac)
    names = []
    for i, (nm, _, _) in enumerate(pairs):
        names += [nm, nm]
    otext, _, _ = oracle.process_pairs(oidx, seq, off, names, None, 0, "", 8)
    header = "@SQ\tSN:20_slice\tLN:321635\n"
    oflags, _ = oracle_dup_flags(oracle, otext, header)
    ends = sam_primary_ends(otext, ["20_slice"])
    dup = capi.sbl_markdup(lib, ends)
    assert len(dup) == len(oflags) == n_pairs
    assert np.array_equal(dup, oflags), (int(dup.sum()), int(oflags.sum()))
    assert dup.sum() > 0
    return int(dup.sum())


def check_align1(lib, oracle, n_pairs, seed, read_len=150, prefix=EXAMPLE_FA, chain_opt=None):
    """chain_opt: (drop_ratio, mask_level, min_chain_weight, max_chain_extend, max_chain_gap) for the chain filter, both sides"""
    oidx, gidx = oracle.idx_load(prefix), lib.index_load(prefix)
    _, seqs, seq, off = sim_reads(n_pairs, seed, read_len, fasta=prefix)
    opt, oopt = lib.opt_init(), None
    if chain_opt is not None:
        for f, v in zip(("drop_ratio", "mask_level", "min_chain_weight", "max_chain_extend", "max_chain_gap"), chain_opt):
            opt[f] = v
        oopt = oracle.opt_chain(*chain_opt)
    ro, regs, st = lib.align1_batch(gidx, opt, seq, off)
    oro, oregs = oracle.align1_batch(oidx, seq, off, oopt)
    assert np.array_equal(ro, oro)
    for f in REG_FIELDS:
        assert np.array_equal(regs[f], oregs[f]), f
    lib.index_destroy(gidx)
    return len(regs)



def reads_with_inner_repeats(fasta, n, seed, rl=250):
    """reads that carry the same reference segment two or three times, further apart than the band: seeds at EQUAL reference positions that do not merge
    (a second, then a third chain at one position: upstream's order among equal positions, the give-up of the wave kernels' ranked form)"""
    rng = np.random.default_rng(seed)
    ctg = simreads.read_fasta(fasta)
    ref = np.asarray(ctg[0][1] if isinstance(ctg[0], tuple) else ctg[0], dtype=np.uint8)
    out = []
    for _ in range(n):
        copies = int(rng.choice([2, 3, 3]))
        xl = int(rng.integers(25, 45))
        p = int(rng.integers(1000, len(ref) - 1000))
        x = ref[p:p + xl]
        gap = int(rng.integers(105, 125)) if copies == 2 else max(5, (rl - copies * xl) // (copies - 1) - 1)
        parts = []
        for c in range(copies):
            parts.append(x)
            if c + 1 < copies:
                parts.append(rng.integers(0, 4, size=gap).astype(np.uint8))
        s = np.concatenate(parts)[:rl]
        if len(s) < rl:
            s = np.concatenate([s, rng.integers(0, 4, size=rl - len(s)).astype(np.uint8)])
        if rng.random() < 0.5:
            s = (3 - s[::-1]).astype(np.uint8)
        out.append(s)
    return out


def check_align1_reads(lib, oracle, seqs, prefix=EXAMPLE_FA):
    """mem_align1_core on given reads: every region field against the oracle"""
    oidx, gidx = oracle.idx_load(prefix), lib.index_load(prefix)
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    seq = np.concatenate(seqs)
    ro, regs, st = lib.align1_batch(gidx, lib.opt_init(), seq, off)
    oro, oregs = oracle.align1_batch(oidx, seq, off)
    assert np.array_equal(ro, oro)
    for f in REG_FIELDS:
        assert np.array_equal(regs[f], oregs[f]), f
    lib.index_destroy(gidx)
    return len(regs)

def repeat_reference(oracle, dirname, seed=5, n_copies=(300, 70), fam_len=(600, 350), unique=40000, max_div=0.03):
    """Writes a small repeat-rich reference (two planted families at 0-3 % divergence, both strands)
    and its index (built by the oracle) into dirname; returns the prefix.  Reads drawn from it carry
    hundreds to thousands of seeds -- the regime of the wave-per-read chaining kernels."""
    prefix = os.path.join(str(dirname), "repeats.fa")
    if os.path.exists(prefix + ".bwt"):
        return prefix
    rng = np.random.default_rng(seed)
    comp = np.array([3, 2, 1, 0], dtype=np.uint8)
    fams = [rng.integers(0, 4, size=l).astype(np.uint8) for l in fam_len]
    pieces = []
    for f, n in zip(fams, n_copies):
        for _ in range(n):
            c = f.copy()
            m = rng.random(c.size) < rng.random() * max_div
            c[m] = rng.integers(0, 4, size=int(m.sum()))
            if rng.random() < 0.5:
                c = comp[c[::-1]]
            pieces.append(c)
    n_sp = len(pieces) + 1
    spacers = [rng.integers(0, 4, size=max(20, int(unique / n_sp))).astype(np.uint8) for _ in range(n_sp)]
    order = rng.permutation(len(pieces))
    seq = [spacers[0]]
    for k, i in enumerate(order):
        seq += [pieces[i], spacers[k + 1]]
    seq = np.concatenate(seq)
    cut = seq.size * 2 // 3
    with open(prefix, "w") as fh:
        for name, s in (("rep1", seq[:cut]), ("rep2", seq[cut:])):
            fh.write(">%s\n" % name)
            txt = "".join("ACGT"[x] for x in s)
            for i in range(0, len(txt), 60):
                fh.write(txt[i:i + 60] + "\n")
    oracle.idx_build(prefix, save=True)
    return prefix


def sbl_streams_from_bits(text, bits, mate, exclude_dups=True, add_mate_tags=True):
    """The three streams samblaster's writer makes of name-grouped SAM lines and the per-line decisions of the device (SSG_SBL_* bits,
    mate line): 0x400 into FLAG of a duplicate block's lines, MC / MQ from the mate's primary line, both primaries of a discordant pair
    (read 1 first) to the discordant stream, splitter lines with _1 / _2 to the splitter stream -- the emit rules of
    speedseq_amd/host/samblaster_main.cpp, restated here so that a device step can be compared with the oracle's streams line by line."""
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    assert len(lines) == len(bits) == len(mate), (len(lines), len(bits), len(mate))
    f = [l.split("\t", 6) for l in lines]
    main, disc, spl = [], [], []

    def emit(i, flag, patch, suffix):
        l = lines[i]
        if patch or suffix:
            x = f[i]
            l = x[0] + (suffix or "") + "\t" + str(flag) + l[len(x[0]) + 1 + len(x[1]):]
        m = int(mate[i])
        if add_mate_tags and m >= 0:
            if "\tMC:Z:" not in l:
                l += "\tMC:Z:" + f[m][5]
            if "\tMQ:i:" not in l:
                l += "\tMQ:i:" + f[m][4]
        return l

    n, b0 = len(lines), 0
    while b0 < n:
        b1 = b0 + 1
        while b1 < n and f[b1][0] == f[b0][0]:
            b1 += 1
        dup = any(bits[i] & 1 for i in range(b0, b1))
        d1 = d2 = -1
        for i in range(b0, b1):
            flag = int(f[i][1])
            if bits[i] & 2:
                if flag & 0x40:
                    d1 = i
                else:
                    d2 = i
            main.append(emit(i, flag | (0x400 if bits[i] & 1 else 0), bool(bits[i] & 1), None))
        if d1 >= 0 and d2 >= 0:
            for i in (d1, d2):
                disc.append(emit(i, int(f[i][1]) | (0x400 if dup else 0), dup, None))
        for i in range(b0, b1):
            if bits[i] & 4:
                flag = int(f[i][1])
                spl.append(emit(i, flag | (0x400 if dup else 0), True, "_1" if flag & 0x40 else "_2"))
        b0 = b1
    return main, disc, spl


def oracle_streams(oracle, text, header):
    """oracle samblaster (the reference's switches) over header + text: record lines of the three streams"""
    out = oracle.samblaster(header + text)
    rec = lambda t: [l for l in t.split("\n") if l and l[0] != "@"]
    return rec(out), rec(oracle.last_discordants), rec(oracle.last_splitters)


def check_hotpath(lib, oracle, n_pairs, per, read_len, to_dev):
    """ssg_hotpath_dev_ex (the bench's step: alignment, duplicate marking, discordant / splitter classification, all on the device) on
    device-resident reads in n_pairs / per upstream batches, against the oracle's `bwa mem` (one insert-size model per upstream batch)
    + samblaster over the whole input: the records left in HBM, printed, are the oracle's SAM text; their per-line decisions
    (duplicate / discordant / splitter bits, MC / MQ source line) give the oracle's three streams line for line.
    to_dev(numpy array) -> (keep-alive object, device pointer)."""
    from speedseq_amd import capi
    kw = dict(ins_mean=800, ins_std=150) if read_len > 200 else {}
    pairs, seqs, seq, off = sim_reads(n_pairs, seed=41, read_len=read_len, dup_frac=0.1, **kw)
    nb = n_pairs // per
    pb = (np.arange(n_pairs) // per).astype(np.int32)
    gidx, oidx = lib.index_load(EXAMPLE_FA), oracle.idx_load(EXAMPLE_FA)
    opt = lib.opt_init()
    keep = [to_dev(seq), to_dev(off), to_dev(pb)]
    (d_seq, d_off, d_pb) = [k[1] for k in keep]
    summary, dup = capi.hotpath_dev(lib, gidx, opt, n_pairs, read_len, d_seq, d_off, d_pb, nb, 0, True)
    s16, h = capi.hotpath_dev_ex(lib, gidx, opt, n_pairs, read_len, d_seq, d_off, d_pb, nb, 0, keep=True)
    names = []
    for nm, _, _ in pairs:
        names += [nm, nm]
    text = ""
    for b in range(nb):
        lo, hi = 2 * per * b, 2 * per * (b + 1)
        t, _, _ = oracle.process_pairs(oidx, seq[off[lo]:off[hi]], off[lo:hi + 1] - off[lo], names[lo:hi], None, lo, "", 4)
        text += t
    header = "@SQ\tSN:20_slice\tLN:321635\n"
    oflags, marked = oracle_dup_flags(oracle, text, header)
    assert np.array_equal(dup, oflags) and oflags.sum() > n_pairs // 40, (int(dup.sum()), int(oflags.sum()))
    assert int(s16[10]) == text.count("\n") and int(s16[1]) == int(oflags.sum()), (s16, text.count("\n"))
    res, bits, mate = capi.dev_records_download(lib, h, n_pairs)
    gtext, _ = capi.sam_format(lib, gidx, opt, res, names, seq, off, None, "")
    res.close(); capi.dev_records_free(lib, h)
    assert gtext == text                                        # the records the step left in HBM print as the oracle's SAM text
    gm, gd, gs = sbl_streams_from_bits(gtext, bits, mate)
    om, od, os_ = oracle_streams(oracle, text, header)
    assert gm == om and gd == od and gs == os_, (len(gm), len(om), len(gd), len(od), len(gs), len(os_))
    n_disc, n_spl = len(od) // 2, len(os_)
    assert (int(s16[8]), int(s16[9])) == (len(od), n_spl) and n_disc > 0 and (n_spl > 0 or n_pairs < 2000), (s16, n_disc, n_spl)
    return int(s16[10]), int(s16[1]), len(od), n_spl


# ------------------------------------------------------------------------------------------------------------------------------
# seeding against tests/seed_reference.py
# ------------------------------------------------------------------------------------------------------------------------------
_SEED_REFS = {}


def seed_ref(prefix):
    """the reference of an index (doubled text + suffix array by sorting), made once per index in a process"""
    import seed_reference
    if prefix not in _SEED_REFS:
        _SEED_REFS[prefix] = seed_reference.SeedRef.from_index(prefix)
    return _SEED_REFS[prefix]


class SeedTally:
    """what a run compared with tests/seed_reference.py: reads submitted and compared, the reads whose reference list holds an interval of pass 2 / of
    pass 3, the x2 values and the seeds with rid < 0 that the reference saw"""
    def __init__(self):
        self.submitted = self.compared = self.pass2 = self.pass3 = self.neg_rid = self.seeds = 0
        self.x2 = set()
        self.seconds = 0.0   # spent inside tests/seed_reference.py

    def check(self, passes=True):
        assert self.submitted > 0 and self.compared == self.submitted, "%d of %d reads compared with the seeding reference" % (self.compared, self.submitted)
        if passes:
            assert self.pass2 > 0 and self.pass3 > 0, "no read with an interval of pass 2 (%d) or of pass 3 (%d)" % (self.pass2, self.pass3)


def seed_opts(lib, oracle, sopt):
    """(option block of the library, option block of the oracle or None, seed_reference.SeedOpts) with sopt = (min_seed_len, split_factor, split_width, max_occ,
    max_mem_intv); None: the defaults, the blocks untouched"""
    import seed_reference
    opt = lib.opt_init() if lib is not None else None
    if not sopt:
        return opt, None, seed_reference.DEFAULTS
    if opt is not None:
        for k, v in zip(("min_seed_len", "split_factor", "split_width", "max_occ", "max_mem_intv"), sopt):
            opt[k] = v
    return opt, (oracle.opt_seed(*sopt) if oracle is not None else None), seed_reference.SeedOpts(*sopt)


def seed_reference_lists(sref, reads, ropt, tally=None):
    """[(intervals, (n1, n2, n3), seeds)] of every read from tests/seed_reference.py"""
    t0 = time.perf_counter()
    out = []
    for q in reads:
        iv, ps = sref.collect_intv(q, ropt, passes=True)
        out.append((iv, ps, sref.seeds_of(iv, ropt)))
    if tally is not None:
        tally.seconds += time.perf_counter() - t0
    return out


def ref_check_smem(got, q, ropt, sref, tally, who, ctx, want=None):
    """got: INTV_DT rows of one read.  Exact equality of the whole list with the reference's: x0, x1, x2, info and the count."""
    import seed_reference
    tally.submitted += 1
    if want is None:
        want = seed_reference_lists(sref, [q], ropt or seed_reference.DEFAULTS, tally)[0]
    iv, ps, _ = want
    g = [(int(r["x0"]), int(r["x1"]), int(r["x2"]), int(r["info"])) for r in got]
    assert g == iv, ("%s disagrees with the seeding reference" % who, ctx, "got", g, "reference", iv, "passes", ps)
    tally.pass2 += ps[1] > 0
    tally.pass3 += ps[2] > 0
    tally.x2.update(t[2] for t in iv)
    tally.compared += 1


def ref_check_seeds(got, rids, q, ropt, sref, tally, who, ctx, want=None):
    """got: SEED_DT rows (or rows of (rbeg, qbeg, len, rid) when rids is None) of one read.  rbeg, qbeg, len, rid equal the reference's, in order."""
    import seed_reference
    tally.submitted += 1
    if want is None:
        want = seed_reference_lists(sref, [q], ropt or seed_reference.DEFAULTS, tally)[0]
    iv, ps, sd = want
    if rids is None:
        g = [tuple(int(x) for x in r) for r in got]
    else:
        g = [(int(r["rbeg"]), int(r["qbeg"]), int(r["len"]), int(k)) for r, k in zip(got, rids)]
    assert g == sd, ("%s disagrees with the seeding reference" % who, ctx, "got", len(g), "reference", len(sd), [x for x in zip(g, sd) if x[0] != x[1]][:4])
    tally.pass2 += ps[1] > 0
    tally.pass3 += ps[2] > 0
    tally.x2.update(t[2] for t in iv)
    tally.neg_rid += sum(1 for t in sd if t[3] < 0)
    tally.seeds += len(sd)
    tally.compared += 1


PLANTED_FAMILIES = (10, 11, 19, 20, 21, 39, 40, 41, 100, 520, 1003)   # copies, both strands together: x2 of a read inside the family


def planted_reference(oracle, dirname, seed=9):
    """Writes a reference of three contigs with families of IDENTICAL copies on both strands and its index (built by the oracle) into dirname; returns
    (prefix, what was planted).  A family of k copies is one random stretch F (40 bases, 30 for the two large families) planted k times as A F A or
    its reverse complement, so every occurrence of F in the doubled text reads A F A: a read that carries C F C matches F and not a base more, and its
    interval has x2 == k.  k lands on both sides of split_width (10, 11), max_mem_intv (19, 20, 21), of -c 20 (20, 21, 39, 40, 41, 100: step 1, 1, 1, 2,
    2, 5) and of the default -c (520, 1003).  The middle 24 bases of each family up to 41 copies are planted 5 more times, so that a re-seeding finds them.
    Further: a tandem repeat of a 7-base unit (30 units); a stretch that is its own reverse complement (60 bases); for the list-capacity cases every
    20-base window of one random 330-base string R, each between bases that R does not continue with (the read R has an interval at every start); a run
    of 30 N in the FASTA, which the index turns into random bases plus an .amb hole."""
    prefix = os.path.join(str(dirname), "planted.fa")
    rng = np.random.default_rng(seed)
    comp = lambda a: (3 - a[::-1]).astype(np.uint8)
    rnd = lambda n: rng.integers(0, 4, size=int(n)).astype(np.uint8)
    A = np.zeros(1, dtype=np.uint8)
    fams, units = {}, []
    for k in PLANTED_FAMILIES:
        F = rnd(30 if k > 100 else 40)
        while F[0] == 0 or F[-1] == 0 or F[0] == 3 or F[-1] == 3:    # (the flanks stay distinguishable on both strands)
            F = rnd(F.size)
        fams[k] = F
        u = np.concatenate([A, F, A])
        units += [u if rng.random() < 0.5 else comp(u) for _ in range(k)]
        if k <= 41:
            c = np.concatenate([A, F[8:32], A])
            units += [c if rng.random() < 0.5 else comp(c) for _ in range(5)]
    R = rnd(330)
    for j in range(R.size - 20 + 1):
        before = (R[j - 1] + 1 + rng.integers(0, 3)) % 4 if j > 0 else rng.integers(0, 4)
        after = (R[j + 20] + 1 + rng.integers(0, 3)) % 4 if j + 20 < R.size else rng.integers(0, 4)
        units.append(np.concatenate([[before], R[j:j + 20], [after]]).astype(np.uint8))
    order = rng.permutation(len(units))
    tandem = np.tile(rnd(7), 30)
    half = rnd(30)
    selfrc = np.concatenate([half, comp(half)])
    pieces = [rnd(400)]
    for i in order:
        pieces += [units[i], rnd(rng.integers(4, 10))]
    pieces += [rnd(300), tandem, rnd(300), selfrc, rnd(400)]
    seq = np.concatenate(pieces)
    cuts = (seq.size // 3, seq.size * 2 // 3)
    ctgs = [seq[:cuts[0]], seq[cuts[0]:cuts[1]], seq[cuts[1]:]]
    n_at = 200                                                      # the N run, inside the first contig's leading random stretch
    meta = dict(families=fams, tandem=tandem, selfrc=selfrc, many=R, ctg_len=[c.size for c in ctgs], n_run=(n_at, 30))
    if not os.path.exists(prefix + ".bwt"):
        with open(prefix, "w") as fh:
            for name, c in zip(("pl1", "pl2", "pl3"), ctgs):
                txt = "".join("ACGT"[x] for x in c)
                if name == "pl1":
                    txt = txt[:n_at] + "N" * 30 + txt[n_at + 30:]
                fh.write(">%s\n" % name)
                for i in range(0, len(txt), 60):
                    fh.write(txt[i:i + 60] + "\n")
        oracle.idx_build(prefix, save=True)
    return prefix, meta


def fixed_seed_reads(sref, seed, planted=None, n_sim=0, fasta=None):
    """The reads a simulation only meets by chance, as (name, codes), from the reference's own text (sref: a seed_reference.SeedRef): lengths 0 (the shortest
    the entry points take), 1, 18, 19, 20, 21 and 310; all N; an N at the first base, at the last base, every 20th base (runs of exactly 19) and every 19th
    (runs of 18); an exact copy of the text; a mismatch every 10 bases; matches of exactly 27 and 28 bases between mismatches; the first and the last 150 bases
    of each strand; reads across the strand junction (one of them its own reverse complement) and, with more than one contig, across a contig boundary;
    planted: a read inside each planted family (C F C between random bases), the self-reverse-complement stretch, the tandem repeat, and the read with an
    interval at every start (310 bases of it, and 100; named many*: their lists outgrow the capacities, so they run in batches of their own)."""
    rng = np.random.default_rng(seed)
    t2, l = sref.t2, sref.l_pac
    rnd = lambda n: rng.integers(0, 4, size=int(n)).astype(np.uint8)
    out = []
    if n_sim:
        _, seqs, _, _ = sim_reads(n_sim // 2, seed, 150, fasta=fasta)
        for i, s in enumerate(seqs):
            s = s.copy()
            if i % 2:
                s[rng.random(s.size) < 0.03] = 4
            out.append(("sim%d" % i, s))
    base = int(l * 0.37)                                             # 310 bases of the forward strand in which every 16-mer occurs once: the copies below match there alone
    while not all(sref.occ(t2[base + j:base + j + 16]) == 1 for j in range(0, 310 - 15, 7)):
        base += 37
        assert base + 310 <= l, "no stretch of unique sequence in this text"
    copy = lambda n, at=base: t2[at:at + n].copy()
    for n in (0, 1, 18, 19, 20, 21, 310):
        out.append(("len%d" % n, copy(n)))
    out.append(("allN", np.full(60, 4, dtype=np.uint8)))
    q = copy(150); q[0] = 4; out.append(("N_first", q))
    q = copy(150); q[-1] = 4; out.append(("N_last", q))
    q = copy(150); q[19::20] = 4; out.append(("N_every20", q))
    q = copy(150); q[18::19] = 4; out.append(("N_every19", q))
    out.append(("exact", copy(150)))
    q = copy(150); q[9::10] = (q[9::10] + 1) % 4; out.append(("mm_every10", q))
    q = copy(150)
    for p in (27, 56, 84, 113):
        q[p] = (q[p] + 2) % 4
    out.append(("runs27_28", q))
    out.append(("fwd_first", t2[:150].copy())); out.append(("fwd_last", t2[l - 150:l].copy()))
    out.append(("rev_first", t2[l:l + 150].copy())); out.append(("rev_last", t2[2 * l - 150:].copy()))
    out.append(("junction_selfrc", t2[l - 75:l + 75].copy())); out.append(("junction", t2[l - 100:l + 50].copy()))
    for k in range(1, len(sref.ctg_off)):
        b = sref.ctg_off[k]
        out.append(("boundary%d" % k, t2[b - 70:b + 80].copy()))
    if planted is not None:
        C = np.ones(1, dtype=np.uint8)
        for k, F in planted["families"].items():
            out.append(("family%d" % k, np.concatenate([rnd(12), C, F, C, rnd(12)])))
            out.append(("family%d_rc" % k, (3 - np.concatenate([rnd(12), C, F, C, rnd(12)])[::-1]).astype(np.uint8)))
        out.append(("selfrc", np.concatenate([rnd(20), planted["selfrc"], rnd(20)])))
        out.append(("tandem", planted["tandem"][3:3 + 120].copy()))
        out.append(("tandem_mm", np.concatenate([rnd(15), planted["tandem"][:90], rnd(15)])))
        out.append(("many310", planted["many"][:310].copy()))
        out.append(("many100", planted["many"][5:105].copy()))
    return out


def cat_reads(reads):
    seqs = [np.ascontiguousarray(q, dtype=np.uint8) for _, q in reads]
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return seqs, np.concatenate(seqs), off
