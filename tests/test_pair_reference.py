"""The paired-end decision stage (mem_pestat, mem_mark_primary_se, mem_pair, mem_approx_mapq_se, mem_sam_pe's decision, mem_reg2sam's record list)
against tests/pair_reference.py: exact arithmetic, definitions instead of loops, nothing shared with csrc/k_pair.h, csrc/k_pairw.h or oracle/orc_pair.c
but the constants and the tie-breaking hash.

Three legs:
  * the reference against itself: hand-worked values, `pair' against a brute-force walk, `pestat' on lists whose quartiles are obvious;
  * the oracle (orc_api_pestat / orc_api_pair_final) and the library (ssg_dbg_pestat / ssg_dbg_pair_final) on CONSTRUCTED region lists, each group of which
    says which branch it aims at, the library in every form: defaults (lane in LDS up to 6 regions a pair, lane on global memory up to 16, wave beyond),
    SSG_PAIR_LDS=0, SSG_PAIR_WAVE_MIN=0, and both lane forms off for the pairs the wave form would take.  The emulation build here; the HIP build in the
    `gpu' twins, which are the only tests that run the device's log and erfc;
  * the product path without a test entry: simulated reads on the repeat-rich reference, regions from align1_batch, mem_process_pairs without mate rescue.

Comparison rule, everywhere: integers and flags equal; avg equal to the correctly rounded exact mean (sums of insert sizes are exact below 2^53 and the
division rounds once); std within ((n + 4) / 2 + avg / std + 2) * 2^-53 relative, n the insert sizes inside the 2-IQR fences: the sum of squares takes
n + 4 roundings of 2^-53 each, the rounded mean enters every term (v - avg)^2 with relative weight 2 * (2^-53 avg) / std at most, the square root halves
the sum of both and adds a rounding of its own, and so does the division.  A result that depends on a NEAR truncation site (pair_reference's header) may be
either neighbour's consequence; before anything is compared, every test asserts on the reference alone that near sites are at most 1 in 1000 of those its
inputs evaluate.  The inputs here have none, but for the one case built to sit on one (an orientation at exactly 5 % of the largest), which asserts it."""
import json
import os
from fractions import Fraction as F

import numpy as np
import pytest

import common
import pair_reference as PR
from speedseq_amd import capi

L0, L1 = 40000, 30000           # two contigs: c0 = [0, L0), c1 = [L0, L0 + L1) of the forward strand
L_PAC = L0 + L1
CTG_OFF = [0, L0]
SSG_EOVERFLOW = -75

FORMS = (("default", {}), ("lds_off", {"SSG_PAIR_LDS": "0"}), ("wave", {"SSG_PAIR_WAVE_MIN": "0"}), ("lane_global", {"SSG_PAIR_LDS": "0", "SSG_PAIR_WAVE_MIN": "1000000"}))

TALLY = PR.Sites()              # the sites of the constructed inputs (groups and insert-size cases) the reference has evaluated in this process, each once


# ------------------------------------------------------------------------------------------------------------------------------
# construction
# ------------------------------------------------------------------------------------------------------------------------------
def reg(pos, rev, qb, qe, score, rlen=None, **kw):
    """a region whose forward-strand footprint starts at absolute position pos; rev: it lies on the reverse strand"""
    rlen = rlen if rlen is not None else qe - qb
    assert (pos < L0) == (pos + rlen <= L0) and pos + rlen <= L_PAC, "a region stays inside its contig"
    rb = pos if not rev else 2 * L_PAC - (pos + rlen)
    d = dict(rb=rb, re=rb + rlen, qb=qb, qe=qe, rid=0 if pos < L0 else 1, score=score, truesc=score, seedcov=max(1, (qe - qb) // 2), w=100, seedlen0=19)
    d.update(kw)
    return d


def fr_mate(pos0, dist, qb=0, qe=100, score=100, **kw):
    """a reverse-strand region whose mem_pair / mem_infer_dir distance from a forward region starting at pos0 is dist (orientation FR): its last base is the key"""
    rlen = kw.get("rlen", qe - qb)
    return reg(pos0 + dist - rlen + 1, True, qb, qe, score, **kw)


def arrays(pairs):
    off, rows = [0], []
    for a, b in pairs:
        for l in (a, b):
            rows += l
            off.append(len(rows))
    regs = np.zeros(len(rows), dtype=capi.ALNREG_DT)
    for i, r in enumerate(rows):
        for k, v in r.items():
            regs[i][k] = v
    return np.array(off, dtype=np.int64), regs


def pes_array(models):
    """models: {orientation: (low, high, avg, std)}; the others have failed"""
    pes = np.zeros(4, dtype=capi.PESTAT_DT)
    pes["failed"] = 1
    for d, (lo, hi, avg, std) in models.items():
        pes[d] = (lo, hi, 0, 0, avg, std)
    return pes


FR = {1: (100, 700, 400.0, 50.0)}
DEC = {1: (100, 900, 400.0, 50.0)}
ALL4 = {0: (100, 700, 400.0, 50.0), 1: (100, 700, 400.0, 50.0), 2: (100, 700, 400.0, 50.0), 3: (100, 700, 400.0, 50.0)}


class Group:
    """pairs that share an option block and an insert-size model; aim: the branch they are built for; expect: a function of the reference's
    (marked lists, records, info) per pair that asserts the branch was reached"""

    def __init__(self, name, aim, pairs, pes, opt=None, id0=0, expect=None, forms=None, may_overflow=()):
        self.name, self.aim, self.pairs, self.pes, self.opt, self.id0, self.expect = name, aim, pairs, pes_array(pes), opt or {}, id0, expect
        self.forms = forms or [f for f, _ in FORMS]
        self.may_overflow = may_overflow      # forms that may answer SSG_EOVERFLOW instead (never a different answer)
        self.off, self.regs = arrays(pairs)
        self._ref = None

    def ropt(self):
        return PR.opt_from(None, **self.opt)

    def reference(self):
        """per pair: the list of acceptable (region rows, record rows) -- one entry unless a near site was met; computed once"""
        if self._ref is None:
            ropt = self.ropt()
            rpes = [PR.Pes(int(p["low"]), int(p["high"]), int(p["failed"]), float(p["avg"]), float(p["std"])) for p in self.pes]
            sites, out, infos = PR.Sites(), [], []
            for p in range(len(self.pairs)):
                r0 = PR.regs_from(self.regs[self.off[2 * p]:self.off[2 * p + 1]])
                r1 = PR.regs_from(self.regs[self.off[2 * p + 1]:self.off[2 * p + 2]])
                info = {}
                alts = PR.alternatives(lambda s: PR.pair_final(ropt, r0, r1, rpes, self.id0 + p, L_PAC, CTG_OFF, s, info if s.flips == frozenset() else None), sites)
                out.append([(_ref_rows(a), recs) for a, recs in alts])
                infos.append((alts[0][0], alts[0][1], info))
            assert sites.n == 0 or len(sites.near) * 1000 <= sites.n, (self.name, "near sites", len(sites.near), "of", sites.n)
            if self.expect:
                self.expect(infos)
            TALLY.add(sites)
            self._ref = out
        return self._ref


REG_COLS = ("rb", "re", "qb", "qe", "rid", "score", "sub", "csub", "sub_n", "secondary", "secondary_all", "hash")


def _ref_rows(a):
    return [[tuple(getattr(e, c) for c in REG_COLS) for e in a[i]] for i in range(2)]


def _got_rows(out, off, p):
    return [[tuple(int(e[c]) for c in REG_COLS) for e in out[off[2 * p + i]:off[2 * p + i + 1]]] for i in range(2)]


def _got_recs(req, req_off, off, p):
    return [[(int(q[0]), int(q[1]) - int(off[2 * p + i]) if q[1] >= 0 else -1, int(q[2]), int(q[3]), int(q[4])) for q in req[req_off[2 * p + i]:req_off[2 * p + i + 1]]] for i in range(2)]


def compare(group, out, req_off, req, who):
    """the stage's lists and records of every pair against the reference's"""
    ref = group.reference()
    if req.dtype.names:
        req = np.stack([req[c] for c in ("kind", "reg", "owner", "flag", "mapq")], axis=1)
    for p in range(len(group.pairs)):
        got = (_got_rows(out, group.off, p), _got_recs(req, req_off, group.off, p))
        assert any(got[0] == rows and got[1] == recs for rows, recs in ref[p]), \
            "%s disagrees with the pairing reference: group %s (%s), pair %d\n got  %s\n %s\n want %s\n %s" % (who, group.name, group.aim, p, got[1], got[0], ref[p][0][1], ref[p][0][0])


class World:
    """the two-contig reference the constructed lists live on, as the library's and the oracle's index"""
    _cache = {}

    @classmethod
    def get(cls, lib, oracle, tmp):
        key = lib.path
        if key not in cls._cache:
            fa = os.path.join(str(tmp), "pairref.fa")
            rng = np.random.default_rng(20261018)
            with open(fa, "w") as f:
                for name, n in (("c0", L0), ("c1", L1)):
                    f.write(">%s\n" % name)
                    s = "".join("ACGT"[c] for c in rng.integers(0, 4, size=n))
                    for i in range(0, n, 80):
                        f.write(s[i:i + 80] + "\n")
            w = cls()
            w.idx = lib.index_build_fasta(fa)
            w.oidx = oracle.idx_build(fa, save=False) if oracle is not None else None
            cls._cache[key] = w
        return cls._cache[key]


def lib_opt(lib, group):
    opt = lib.opt_init()
    for k, v in group.opt.items():
        opt[k] = v
    if "a" in group.opt or "b" in group.opt:
        m = opt["mat"][0]
        for x in range(4):
            for y in range(4):
                m[x * 5 + y] = opt["a"][0] if x == y else -opt["b"][0]
    return opt


def run_library(lib, world, group, monkeypatch, who):
    """the group through ssg_dbg_pair_final in every form it is meant for; returns {form: 'ok' | 'overflow'}"""
    outcome = {}
    opt = lib_opt(lib, group)
    for form, env in FORMS:
        if form not in group.forms:
            continue
        for k in ("SSG_PAIR_LDS", "SSG_PAIR_WAVE_MIN"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        try:
            out, req_off, req = lib.dbg_pair_final(world.idx, opt, group.id0, group.off, group.regs, group.pes)
        except capi.SsgError as e:
            assert form in group.may_overflow and ("error %d" % SSG_EOVERFLOW) in str(e), (who, group.name, form, str(e))
            outcome[form] = "overflow"
            continue
        compare(group, out, req_off, req, "%s, form %s" % (who, form))
        outcome[form] = "ok"
    return outcome


def run_oracle(oracle, world, group):
    oopt = None
    if group.opt:
        import ctypes as C
        oopt = C.c_void_p(oracle.l.orc_api_opt_new())
        o = group.ropt()
        oracle.l.orc_api_opt_scores(oopt, C.c_int(o["a"]), C.c_int(o["b"]), C.c_int(o["o_del"]), C.c_int(o["e_del"]), C.c_int(o["o_ins"]), C.c_int(o["e_ins"]))
        oracle.l.orc_api_opt_pair(oopt, C.c_int(o["flag"]), C.c_int(o["max_XA_hits"]), C.c_float(o["mapQ_coef_len"]), C.c_int(o["mapQ_coef_fac"]), C.c_int(o["T"]), C.c_int(o["pen_unpaired"]))
    out, req_off, req = oracle.pair_final(world.oidx, group.id0, group.off, group.regs, group.pes, oopt)
    compare(group, out, req_off, req, "the oracle")


# ------------------------------------------------------------------------------------------------------------------------------
# the groups
# ------------------------------------------------------------------------------------------------------------------------------
def _recs_main(recs, i):
    return [r for r in recs[i] if r[0] == PR.MAIN]


def g_tie_by_hash():
    """equal pair scores decided by the hash: read 2 has two identical regions, one k std below the mean insert size and one k std above; 48 pair ids"""
    pairs = []
    for t in range(48):
        k = 1 + t % 3
        p0 = 1000 + 37 * t
        pairs.append(([reg(p0, False, 0, 100, 100)], [fr_mate(p0, 400 - 50 * k), fr_mate(p0, 400 + 50 * k)]))

    def expect(infos):
        tied = [i["tied"] for _, _, i in infos]
        zs = {(a[1][recs[1][0][1]].rb > a[1][1 - recs[1][0][1]].rb) for a, recs, _ in infos}
        assert all(tied) and zs == {True, False}, "both outcomes of the tie must occur"
    return Group("tie_by_hash", g_tie_by_hash.__doc__, pairs, FR, id0=3, expect=expect)


def _close_second(p0):
    """read 1 of a pair whose own MAPQ is small (a shadowed hit 3 below the best, far away: q_se = 5), so that the pair's q_pe shows in the record"""
    return [reg(p0, False, 0, 100, 100), reg(p0 + 20000, False, 0, 100, 97)]


def g_dist_bounds():
    """dist at low - 1, low, high, high + 1 (6 std from the mean: paired with q_pe = 18, or not paired and MAPQ 5); a stronger mate just outside next to a
    weaker one inside"""
    pairs = []
    for j, d in enumerate((99, 100, 700, 701)):
        pairs.append((_close_second(2000 + 1000 * j), [fr_mate(2000 + 1000 * j, d)]))
    for j, (d_out, d_in) in enumerate(((701, 700), (99, 100), (701, 400))):
        p0 = 8000 + 1000 * j
        pairs.append((_close_second(p0), [fr_mate(p0, d_out, score=100), fr_mate(p0, d_in, score=98)]))

    def expect(infos):
        n = [i.get("n_cand", 0) for _, _, i in infos]
        assert n == [0, 1, 1, 0, 1, 1, 1], n
        q = [recs[0][0][4] for _, recs, _ in infos]
        assert q[:4] == [5, 18, 18, 5] and all(x > 5 for x in q[4:]), q
    return Group("dist_bounds", g_dist_bounds.__doc__, pairs, FR, expect=expect)


def g_q_rounding(k, target):
    """a candidate whose q lies 5e-4 under the point where (int)(x + .499) and (int)(x + .5) part: the insert-size term is target = -n - .4995 at a distance
    of 200 from the mean, by the choice of std (bisection on z, std = 200 / z); seen through q_pe on a read whose own MAPQ is 5.  Three regions (lane forms)
    and nineteen (wave form by default)"""
    import math
    lo, hi = 0.0, 30.0
    for _ in range(200):
        z = (lo + hi) / 2
        if 0.721 * math.log(2.0 * math.erfc(z * PR.SQRT1_2)) > target:
            lo = z
        else:
            hi = z
    std = 200.0 / z
    p0 = 6000
    junk = [reg(p0 + 15000 + 100 * j, True, 0, 100, 20) for j in range(16)]
    pairs = [(_close_second(p0), [fr_mate(p0, 600)]), (_close_second(p0), [fr_mate(p0, 600)] + junk), (_close_second(p0), [fr_mate(p0, 200)] + junk[:5])]

    def expect(infos):
        m = PR.Pes(100, 900, 0, 400.0, std)
        st = PR.Sites()
        q = PR.pair_score(PR.opt_from(), 100, 100, 600, m, st)
        x = 200 + PR.MP.mpf(0.721) * PR.MP.log(2 * PR.MP.erfc(PR.MP.mpf(200.0 / std) * PR.SQRT1_2))
        assert int(x + 0.5) == q + 1 and 1e-6 < st.min_margin < 1e-5 and not st.near, (q, x, st.min_margin)
        assert all(info.get("branch") == "paired" and recs[0][0][4] == PR.raw_mapq(PR.opt_from(), q - 183, PR.Sites()) < 45 for _, recs, info in infos)
    return Group("q_rounding_%d" % k, g_q_rounding.__doc__, pairs, {1: (100, 900, 400.0, std)}, expect=expect)


def g_failed_orientations():
    """one, two and three failed orientations: both reads have a hit on each strand, so that every orientation class has a candidate"""
    out = []
    masks = [(0,), (1,), (2,), (3,), (0, 1), (1, 2), (0, 3), (1, 3), (0, 1, 2), (1, 2, 3), (0, 2, 3), (0, 1, 3)]
    for failed in masks:
        pes = {d: m for d, m in ALL4.items() if d not in failed}
        pairs = []
        for t in range(3):
            p0 = 3000 + 2500 * t
            # read 1: forward at p0, reverse at p0 + 900; read 2: forward at p0 + 350, reverse ending 420 after p0; the query intervals do not overlap
            pairs.append(([reg(p0, False, 0, 60, 60 - t), reg(p0 + 900, True, 70, 130, 58)], [reg(p0 + 350, False, 0, 60, 59), fr_mate(p0, 420, 70, 130, 57 + t)]))
        out.append(Group("failed_%s" % "".join(map(str, failed)), g_failed_orientations.__doc__, pairs, pes, opt=dict(T=80)))
    return out


def g_junction_and_contigs():
    """regions on both strands next to the strand junction (rb >= l_pac); two contigs whose hits come closer than `high' once the contig offset is subtracted,
    and closer than `high' across the contig boundary"""
    pairs = []
    e = L_PAC - 100                                             # the last 100 bases of c1: forward rb just below l_pac, reverse rb just above it
    pairs.append(([reg(e - 400, False, 0, 100, 100)], [reg(e, True, 0, 100, 100)]))              # FR across nothing: dist 499
    pairs.append(([reg(e, False, 0, 100, 100)], [reg(e - 300, True, 0, 100, 100)]))              # RF: the reverse hit lies before the forward one
    pairs.append(([reg(e, True, 0, 100, 100)], [reg(e - 400, False, 0, 100, 100)]))              # the same as the first, reads swapped
    pairs.append(([reg(0, True, 0, 100, 100)], [reg(350, True, 0, 100, 100)]))                   # RR / FF on the reverse strand at the far end (rb near 2 l_pac)
    pairs.append(([reg(500, False, 0, 100, 100)], [fr_mate(L0 + 500, 200)]))                     # offsets in the contigs 200 apart, contigs differ
    pairs.append(([reg(L0 - 250, False, 0, 100, 100)], [fr_mate(L0 - 250, 400)]))                # 400 apart on the doubled strand, across the contig boundary
    pairs.append(([reg(L0 + 600, False, 0, 100, 100), reg(600, False, 0, 100, 99)], [fr_mate(600, 400), fr_mate(L0 + 600, 380, score=98)]))   # a proper mate on each contig

    def expect(infos):
        n = [i.get("n_cand", 0) for _, _, i in infos]
        assert n[4] == 0 and n[5] == 0 and n[6] == 2 and n[0] == 1 and n[2] == 1, n
    return Group("junction_and_contigs", g_junction_and_contigs.__doc__, pairs, ALL4, expect=expect)


def _mapq_reads():
    """single reads for mem_approx_mapq_se: (regions, what)"""
    reads = []
    for l in (30, 49, 50, 51, 100, 150, 250):
        for frac in (1.0, 0.97, 0.9, 0.8):
            score = max(30, int(l * frac))
            for frac_rep in (0.0, 0.25, 0.999):
                reads.append([reg(5000, False, 0, l, score, frac_rep=frac_rep)])                                       # sub == 0
                reads.append([reg(5000, False, 0, l, score, frac_rep=frac_rep, csub=score - 7)])                       # csub > sub
                reads.append([reg(5000, False, 0, l, score, frac_rep=frac_rep), reg(9000, False, 0, l, score - 3)])     # sub from a shadowed hit, sub_n 1
            reads.append([reg(5000, False, 0, l, score), reg(9000, False, 0, l, score)])                               # sub >= score
            reads.append([reg(5000, False, 0, l, score, csub=score)])                                                  # csub >= score
            reads.append([reg(5000, False, 0, l, score, rlen=l + 9)])                                                  # the reference span is the longer one
    for sub_n in range(0, 21):
        reads.append([reg(5000, False, 0, 150, 150, sub_n=sub_n)])                                                     # clamp at 60 and the sub_n term
        reads.append([reg(5000, False, 0, 150, 120, sub_n=sub_n), reg(9000, False, 0, 150, 112)])                      # sub_n + 1 through the scan, towards the clamp at 0
        reads.append([reg(5000, False, 0, 60, 45, sub_n=sub_n)])
        reads.append([reg(5000, False, 0, 150, 120, sub_n=sub_n), reg(9000, False, 0, 150, 118)])                      # 4 - the sub_n term: below 0 from sub_n = 1 on
    return reads


def g_mapq():
    """mem_approx_mapq_se through the no-pairing branch (every orientation failed): sub == 0, csub > sub, sub >= score, l below / at / above mapQ_coef_len,
    sub_n 0..20, frac_rep 0 / 0.25 / 0.999, the clamps at 0 and 60"""
    reads = _mapq_reads()
    pairs = [(reads[i], reads[(i + 1) % len(reads)]) for i in range(0, len(reads), 2)]

    def expect(infos):
        qs = {r[4] for _, recs, _ in infos for i in range(2) for r in recs[i]}
        assert 0 in qs and 60 in qs and len(qs) > 30, sorted(qs)
    return Group("mapq", g_mapq.__doc__, pairs, {}, expect=expect)


def g_mapq_coef0():
    """mapQ_coef_len == 0: the seed-coverage formula and its identity < 0.95 branch (score below 0.75 l at a = 1, b = 4), on both sides of 0.95"""
    reads = []
    for l in (40, 100, 150):
        for score in (l, l - 4, l - 9, l - 24, int(0.75 * l) + 1, int(0.75 * l), int(0.75 * l) - 1, int(0.7 * l), int(0.6 * l)):
            if score < 31:
                continue
            for cov in (19, l // 2, l):
                reads.append([reg(5000, False, 0, l, score, seedcov=cov), reg(9000, False, 0, l, max(20, score - 30))])
                reads.append([reg(5000, False, 0, l, score, seedcov=cov, frac_rep=0.25)])
    pairs = [(reads[i], reads[(i + 1) % len(reads)]) for i in range(0, len(reads), 2)]

    def expect(infos):
        o = PR.opt_from(None, mapQ_coef_len=0.0)
        low = high = changed = 0
        for a, recs, _ in infos:
            for i in range(2):
                r = a[i][0]
                l = max(r.qe - r.qb, r.re - r.rb)
                identity = 1 - F(l * o["a"] - r.score, o["a"] + o["b"]) / l
                assert recs[i][0][1] == 0 and recs[i][0][4] == PR.mapq_se(o, r)
                if identity < F(0.95):
                    low += 1
                    changed += PR.mapq_se(dict(o, b=10 ** 6), r) != recs[i][0][4]      # b huge: identity 1, the branch not taken
                else:
                    high += 1
        assert low >= 20 and high >= 20 and changed >= 10, (low, high, changed)
    return Group("mapq_coef0", g_mapq_coef0.__doc__, pairs, {}, opt=dict(mapQ_coef_len=0.0), expect=expect)


def g_decision_tree():
    """q_pe above q_se + 40; o <= score_un; is_multi on either read; XA lists at max_XA_hits and one more; z[i] a secondary (the rewiring)"""
    pairs, what = [], []
    p0 = 4000
    # q_pe above q_se + 40: read 1's hit has a close second (q_se small) that has no mate, the pair is unique
    pairs.append(([reg(p0, False, 0, 100, 100), reg(p0 + 20000, False, 0, 100, 97)], [fr_mate(p0, 400)])); what.append("q_pe_cap")
    # o <= score_un: the insert size is 6.8 / 8 std off: .721 ln(2 erfc) = -18.2 / -24.7, more than pen_unpaired
    pairs.append(([reg(p0, False, 0, 100, 100)], [fr_mate(p0, 740)])); what.append("o_le_score_un")
    pairs.append(([reg(p0, False, 0, 100, 100)], [fr_mate(p0, 800)])); what.append("o_le_score_un")
    # is_multi on read 1, on read 2
    pairs.append(([reg(p0, False, 0, 70, 70), reg(p0 + 9000, False, 80, 150, 66)], [fr_mate(p0, 400, 0, 150, 150)])); what.append("multi0")
    pairs.append(([reg(p0, False, 0, 150, 150)], [fr_mate(p0, 400, 0, 70, 70), reg(p0 + 9000, True, 80, 150, 50)])); what.append("multi1")
    pairs.append(([reg(p0, False, 0, 70, 70), reg(p0 + 9000, False, 80, 150, 29)], [fr_mate(p0, 400, 0, 150, 150)])); what.append("second_below_T")
    # XA lists: 5 and 6 shadowed hits within XA_drop_ratio, and one below it
    for n_xa in (4, 5, 6):
        shadow = [reg(p0 + 3000 * (j + 1), False, 0, 100, 95 - j) for j in range(n_xa)] + [reg(p0 + 30000, False, 0, 100, 60)]
        pairs.append(([reg(p0, False, 0, 100, 100)] + shadow, [fr_mate(p0, 400)])); what.append("xa%d" % n_xa)
        pairs.append(([reg(p0, False, 0, 100, 100)] + shadow, [])); what.append("xa%d_single" % n_xa)
    # the csub cap: the pair's MAPQ is 48 (q_se 8 + 40), raw_mapq(score - csub) = 18 cuts it; on read 1, then on read 2
    pairs.append(([reg(p0, False, 0, 100, 100, csub=97)], [fr_mate(p0, 400)])); what.append("csub_cap0")
    pairs.append(([reg(p0, False, 0, 100, 100)], [fr_mate(p0, 400, csub=97)])); what.append("csub_cap1")
    # z[i] a secondary: read 1's best hit has no mate, its shadowed second has one
    pairs.append(([reg(p0 + 20000, False, 0, 100, 100), reg(p0, False, 0, 100, 96), reg(p0 + 25000, False, 0, 100, 90)], [fr_mate(p0, 400)])); what.append("rewire")
    pairs.append(([reg(p0, False, 0, 100, 100)], [reg(p0 + 22000, True, 0, 100, 100), fr_mate(p0, 410, score=97), reg(p0 + 26000, True, 10, 100, 85)])); what.append("rewire")

    def expect(infos):
        for (a, recs, info), w in zip(infos, what):
            m0, m1 = _recs_main(recs, 0), _recs_main(recs, 1)
            if w == "q_pe_cap":
                assert info.get("branch") == "paired" and m0[0][3] & 2 and m0[0][4] < 60 and m1[0][4] == 60, (w, recs)
            elif w == "o_le_score_un":
                assert info.get("branch") == "paired" and not m0[0][3] & 2, (w, recs)
            elif w.startswith("multi"):
                i = int(w[-1])
                assert info.get("branch") != "paired" and len(_recs_main(recs, i)) == 2 and _recs_main(recs, i)[1][3] & 0x800, (w, recs)
            elif w.startswith("xa") and not w.endswith("single"):
                n = sum(1 for r in recs[0] if r[0] == PR.XA)
                assert n == (int(w[2]) if int(w[2]) <= 5 else 0), (w, recs)
            elif w.startswith("csub_cap"):
                i = int(w[-1])
                assert info.get("branch") == "paired" and _recs_main(recs, i)[0][4] == 18 and _recs_main(recs, 1 - i)[0][4] == 60, (w, recs)
            elif w == "rewire":
                i = 0 if len(a[0]) > 1 else 1
                assert info.get("branch") == "paired" and _recs_main(recs, i)[0][1] == 1 and a[i][1].secondary == -2 and a[i][0].secondary_all == 1, (w, recs)
    return Group("decision_tree", g_decision_tree.__doc__, pairs, DEC, expect=expect)


def g_flags(flag, name):
    """-M (supplementary lines carry 0x10000) and -P (no pairing): the decision-tree group's pairs again"""
    g = g_decision_tree()
    return Group(name, g_flags.__doc__, g.pairs, DEC, opt=dict(flag=flag))


def g_form_boundaries():
    """the default split at its own boundaries: 6 / 7 regions in all (LDS slice), 15 / 16 / 17 (lane / wave), the regions divided between the reads in every
    way the LDS slice could mis-size (0 + n, 1 + (n - 1), halves)"""
    rng = np.random.default_rng(5)
    pairs = []
    for tot in (5, 6, 7, 8, 15, 16, 17, 18):
        for n0 in sorted({0, 1, tot // 2, tot - 1, tot}):
            p0 = int(rng.integers(2000, 30000))
            a = [reg(p0 + int(rng.integers(0, 300)), False, int(rng.integers(0, 50)), int(rng.integers(60, 150)), int(rng.integers(31, 60))) for _ in range(n0)]
            b = [fr_mate(p0, int(rng.integers(90, 720)), int(rng.integers(0, 50)), int(rng.integers(60, 150)), int(rng.integers(31, 60))) for _ in range(tot - n0)]
            pairs.append((a, b))
    return Group("form_boundaries", g_form_boundaries.__doc__, pairs, FR, id0=77)


def _sub_n_term(n):
    return int(4.343 * np.log(n + 1) + .499) if n > 0 else 0


def _heavy_pair(rng, p0, n0, n1, equal_q=False, few=False, near=None):
    """Long lists that are still printed as a pair, with mem_pair's o, sub and n_sub visible in the record.  Every region of a read covers nearly the whole
    query, so a read has one primary and the rest is shadowed by it (no is_multi).  Each read has: a far hit of 103 without a mate (it makes the read's own
    MAPQ 0 .. 2, so that q_pe shows), the hit of the best pair (104, the two at the mean insert size: o = 208), read 2 a hit of 98 at the mean as well (the
    runner-up: sub = 202), and a crowd around them: q_pe = raw_mapq(6) - the n_sub term = 36 - (3 .. 30).  The crowd scores 90 .. 98 (hundreds of candidates
    within the largest penalty of the runner-up), or, with near = k, 60 .. 80 but for k hits of each read (a handful within it, where one candidate more or
    less changes the term).  equal_q: few distinct scores and distances, so that many candidates share a q; few: all but three of read 2's crowd lie
    beyond `high'."""
    def q_iv():
        return int(rng.integers(0, 8)), int(rng.integers(143, 151))

    def score(j):
        if near is not None and j >= near:
            return int(rng.choice([62, 70, 80])) if equal_q else int(rng.integers(60, 81))
        return int(rng.choice([91, 95, 98])) if equal_q else int(rng.integers(90, 99))
    a = [reg(p0 + 20000, False, 0, 150, 103), reg(p0, False, 0, 150, 104)]
    b = [reg(p0 + 25000, True, 0, 150, 103), fr_mate(p0, 400, 0, 150, 104), fr_mate(p0, 400, 1, 150, 98)]
    for j in range(n0 - 2):
        qb, qe = q_iv()
        a.append(reg(p0 + (int(rng.integers(0, 4)) * 50 if equal_q else int(rng.integers(0, 300))), False, qb, qe, score(j)))
    for j in range(n1 - 3):
        qb, qe = q_iv()
        d = 400 + (int(rng.integers(-3, 4)) * 50 if equal_q else int(rng.integers(-320, 330)))
        if few and j >= 3:
            d = 5000 + int(rng.integers(0, 2000))
        b.append(fr_mate(p0, d, qb, qe, score(j)))
    order = rng.permutation(len(a)); a = [a[i] for i in order]
    order = rng.permutation(len(b)); b = [b[i] for i in order]
    return a, b


def _expect_pairing_visible(infos, what):
    """on the reference alone: every pair of the group is printed as a pair, n_sub > 0, and read 1's MAPQ is q_pe = raw_mapq(o - sub) - the n_sub term
    (so o, sub and n_sub all reach a compared field); an n_sub one too large, and one too small, would change that term in several pairs"""
    o = PR.opt_from()
    up = down = edge = 0
    for a, recs, i in infos:
        assert i.get("branch") == "paired" and i["n_sub"] > 0 and i["o"] == 208 and i["sub"] > 191, (what, i)
        q_pe = PR.raw_mapq(o, i["o"] - i["sub"], PR.Sites()) - _sub_n_term(i["n_sub"])
        assert 0 < q_pe < 40 and recs[0][0][4] == q_pe and recs[0][0][3] & 2, (what, i, recs[0][0])
        up += _sub_n_term(i["n_sub"] + 1) != _sub_n_term(i["n_sub"])
        down += _sub_n_term(i["n_sub"] - 1) != _sub_n_term(i["n_sub"])
        edge += i["n_at_edge"] > 0 and _sub_n_term(i["n_sub"] - i["n_at_edge"]) != _sub_n_term(i["n_sub"])
    assert up >= 3 and down >= 3 and edge >= 3, (what, up, down, edge)


def g_wave_heavy():
    """the wave form's own ground: 64 .. 400 regions an end, hundreds to thousands of candidates, many with equal q (the histogram count against the definition
    of n_sub, candidates exactly at the edge of the count included), the best and the runner-up met by the same lane and by different lanes"""
    rng = np.random.default_rng(11)
    pairs = []
    sizes = [(64, 64), (65, 63), (400, 70), (70, 400), (128, 129), (200, 200)] + [(int(rng.integers(64, 160)), int(rng.integers(64, 160))) for _ in range(30)]
    for j, (n0, n1) in enumerate(sizes):
        pairs.append(_heavy_pair(rng, 2000 + 400 * j, n0, n1, equal_q=j % 2 == 0, near=None if j % 4 < 2 else j % 7))
    for j in range(12):                                        # a few candidates only: best and runner-up often in one lane
        pairs.append(_heavy_pair(rng, 2000 + 400 * (len(sizes) + j), 70, 70, few=True))

    def expect(infos):
        same = [i["best_rank"] % 64 == i["second_rank"] % 64 for _, _, i in infos]
        assert sum(same) >= 3 and len(same) - sum(same) >= 3, "best and runner-up in one lane, and in two"
        assert max(i["n_equal_sub"] for _, _, i in infos) > 20 and max(i["n_cand"] for _, _, i in infos) > 2000
        _expect_pairing_visible(infos, "wave_heavy")
    return Group("wave_heavy", g_wave_heavy.__doc__, pairs, FR, id0=1000, expect=expect, forms=["default", "wave"])


def g_mid_lane():
    """17 .. 40 regions a pair through the lane forms as well (the wave form takes them by default): equal q among dozens of candidates"""
    rng = np.random.default_rng(12)
    pairs = [_heavy_pair(rng, 2000 + 400 * j, int(rng.integers(8, 21)), int(rng.integers(9, 21)), equal_q=j % 2 == 0, near=None if j % 4 < 2 else j % 5) for j in range(40)]
    return Group("mid_lane", g_mid_lane.__doc__, pairs, FR, id0=500, expect=lambda infos: _expect_pairing_visible(infos, "mid_lane"))


def g_q_1024(a):
    """scoring a = 2 / 3 with two 300-base reads: q reaches 1024, beyond the wave form's histogram.  Upstream has no such limit: the reference's answer or an
    error return, never another answer"""
    rng = np.random.default_rng(13 + a)
    pairs = []
    for j in range(4):
        n = 3 if j < 2 else 12                                # 6 regions a pair: the lane forms; 24: the wave form by default
        p0 = 3000 + 900 * j
        x, y = [], []
        for _ in range(n):
            qb, qe = int(rng.integers(0, 10)), int(rng.integers(291, 301))
            x.append(reg(p0 + int(rng.integers(0, 200)), False, qb, qe, int(rng.integers(270 * a, (qe - qb) * a + 1))))
            qb, qe = int(rng.integers(0, 10)), int(rng.integers(291, 301))
            y.append(fr_mate(p0, 400 + int(rng.integers(-120, 330)), qb, qe, int(rng.integers(270 * a, (qe - qb) * a + 1))))
        pairs.append((x, y))

    def expect(infos):
        assert all(i["n_cand"] > 0 for _, _, i in infos) and all(recs[0][0][3] & 2 and recs[0][0][0] == PR.MAIN for _, recs, _ in infos)
        assert all(a[0][recs[0][0][1]].score + a[1][recs[1][0][1]].score >= 1060 for a, recs, _ in infos), "q of the best pair is beyond 1024"
    return Group("q_1024_a%d" % a, g_q_1024.__doc__, pairs, FR, opt=dict(a=a, b=4 * a, o_del=6 * a, e_del=a, o_ins=6 * a, e_ins=a, T=30 * a, pen_unpaired=17 * a), expect=expect,
                 may_overflow=("default", "lds_off", "wave"))


def g_random_light():
    """a few thousand light pairs drawn at random: 0 .. 4 regions an end, both strands, both contigs, csub, frac_rep"""
    rng = np.random.default_rng(1)

    def rand_reg(rid, center, rev):
        ql = int(rng.integers(30, 151)); qb = int(rng.integers(0, 151 - ql))
        lo, hi = (0, L0) if rid == 0 else (L0, L_PAC)
        pos = min(max(center + int(rng.integers(-600, 600)), lo + 10), hi - 200)
        return reg(pos, rev, qb, qb + ql, int(rng.integers(20, ql + 1)), rlen=ql + int(rng.integers(-2, 3)), csub=int(rng.integers(0, 40)) if rng.random() < .3 else 0,
                   seedcov=int(rng.integers(10, ql)), frac_rep=float(rng.choice([0, 0, .25, .999])))
    pairs = []
    for _ in range(3000):
        rid = int(rng.integers(0, 2)); c = int(rng.integers(2000, 25000)) + (L0 if rid else 0)
        pairs.append(([rand_reg(rid if rng.random() < .9 else 1 - rid, c, bool(rng.random() < .5)) for _ in range(int(rng.integers(0, 5)))],
                      [rand_reg(rid, c + 300, bool(rng.random() < .5)) for _ in range(int(rng.integers(0, 5)))]))
    return Group("random_light", g_random_light.__doc__, pairs, {1: (50, 900, 431.7, 97.3), 2: (100, 1500, 800.3, 210.9)}, id0=5)


_GROUPS = {}


def groups():
    if not _GROUPS:
        gs = [g_tie_by_hash(), g_dist_bounds(), g_q_rounding(0, -10.4995), g_q_rounding(1, -12.4995), g_q_rounding(2, -14.4995)] + g_failed_orientations() + [g_junction_and_contigs(), g_mapq(), g_mapq_coef0(), g_decision_tree(), g_flags(PR.F_NO_MULTI, "flag_M"),
              g_flags(PR.F_NOPAIRING, "flag_P"), g_form_boundaries(), g_wave_heavy(), g_mid_lane(), g_q_1024(2), g_q_1024(3), g_random_light()]
        for g in gs:
            _GROUPS[g.name] = g
    return _GROUPS


GROUP_NAMES = ["tie_by_hash", "dist_bounds", "q_rounding_0", "q_rounding_1", "q_rounding_2"] + ["failed_%s" % "".join(map(str, m)) for m in [(0,), (1,), (2,), (3,), (0, 1), (1, 2), (0, 3), (1, 3), (0, 1, 2), (1, 2, 3), (0, 2, 3), (0, 1, 3)]] + \
              ["junction_and_contigs", "mapq", "mapq_coef0", "decision_tree", "flag_M", "flag_P", "form_boundaries", "wave_heavy", "mid_lane", "q_1024_a2", "q_1024_a3", "random_light"]


# ------------------------------------------------------------------------------------------------------------------------------
# the reference against itself
# ------------------------------------------------------------------------------------------------------------------------------
def test_reference_hand_worked_values():
    o = PR.opt_from()
    s = PR.Sites()
    # mem_approx_mapq_se: l = 100 >= 50, tmp = 3 / ln 100 = 0.651442..., identity 1: 6.02 * (100 - 19) * 0.424376... = 206.93 -> 207, clamp 60
    assert PR.mapq_se(o, PR.Reg(0, 100, 0, 100, 0, 100), s) == 60
    # l = 40 < 50: identity = 1 - (40 - 35) / 5 / 40 = 0.975; 6.02 * 16 * 0.975^4 = 87.04 -> 87 -> 60; with sub_n = 3: 60 after the clamp?  no: 87 - (int)(4.343 ln 4 + .499 = 6.519) = 81 -> 60
    assert PR.mapq_se(o, PR.Reg(0, 40, 0, 40, 0, 35, sub_n=3), s) == 60
    # sub = 30 through csub: 6.02 * 5 * 0.975^4 = 27.20 -> 27; frac_rep 0.25: 27 * 0.75 + .499 = 20.749 -> 20
    assert PR.mapq_se(o, PR.Reg(0, 40, 0, 40, 0, 35, csub=30), s) == 27
    assert PR.mapq_se(o, PR.Reg(0, 40, 0, 40, 0, 35, csub=30, frac_rep=0.25), s) == 20
    # sub_n = 20: 27 - (int)(4.343 * ln 21 + .499 = 13.721) = 14
    assert PR.mapq_se(o, PR.Reg(0, 40, 0, 40, 0, 35, csub=30, sub_n=20), s) == 14
    assert PR.mapq_se(o, PR.Reg(0, 40, 0, 40, 0, 35, csub=35), s) == 0                       # sub >= score
    # raw_mapq: 6.02 * 17 + .499 = 102.839 -> 102
    assert PR.raw_mapq(o, 17, s) == 102
    # mem_pair's q at the mean: 2 erfc(0) = 2, .721 ln 2 = 0.49976: 200 + 0.49976 + .499 = 200.9988 -> 200 (1.2e-3 from flipping); one std off: 2 erfc(1 / sqrt 2) = 0.63462,
    # .721 ln = -0.32790 -> 200.1711 -> 200; two std: 2 erfc(sqrt 2) = 0.0910, .721 ln = -1.7282 -> 198.77 -> 198; four std: 1.2669e-4 ... -6.4711 -> 194.03 -> 194
    m = PR.Pes(100, 700, 0, 400.0, 50.0)
    assert [PR.pair_score(o, 100, 100, d, m, s) for d in (400, 450, 350, 500, 600)] == [200, 200, 200, 198, 194]
    assert PR.pair_score(o, 3, 2, 700, m, s) == 0                                            # 5 - 12.98 clamps at 0
    with pytest.raises(ArithmeticError):
        PR.pair_score(o, 100, 100, 400 + 50 * 40, m, s)                                      # 40 std: 2 erfc underflows
    assert len(s.near) == 0 and 5e-6 < s.min_margin < 7e-6                                   # the pair at the mean: 1.2e-3 of 200
    # infer_dir: FF, FR, RF, RR
    L = 1000
    assert [PR.infer_dir(L, 100, 300), PR.infer_dir(L, 100, 2 * L - 1 - 300), PR.infer_dir(L, 300, 2 * L - 1 - 100), PR.infer_dir(L, 300, 100)] == [(0, 200), (1, 200), (2, 200), (3, 200)]
    # the hash: hash_64(0) of Thomas Wang's mix
    assert PR.hash_64(0) == 0x6a396cd39c352659 and PR.hash_64(12345) == 0xced1fe8e61c2d2b1   # from a C transcription of the mix, compiled and run


def test_reference_truncation_sites_and_flips():
    s = PR.Sites()
    assert s.trunc(F(5, 2)) == 2 and s.trunc(F(2502, 1000)) == 3 and s.trunc(F(-7, 2)) == -3 and len(s.near) == 0
    x = F(3) - PR.C499 + F(1, 10 ** 12)                         # x + .499 = 3 + 1e-12: near
    s = PR.Sites()
    assert s.trunc(x) == 3 and s.near == [0]
    assert PR.Sites(flips=[0]).trunc(x) == 2
    assert PR.alternatives(lambda st: st.trunc(x) * 10 + st.trunc(F(1, 3))) == [30, 20]
    s = PR.Sites()
    assert s.trunc(lambda: PR.MP.mpf(2) - PR.MP.mpf(PR.C499.numerator) / PR.C499.denominator - PR.MP.mpf(10) ** -13) == 1 and s.near == [0]


def test_reference_pair_against_brute_force():
    rng = np.random.default_rng(2)
    o = PR.opt_from()
    pes = [PR.Pes(100, 700, 0, 400.0, 50.0), PR.Pes(50, 900, 0, 431.7, 97.3), PR.Pes(1, 600, 0, 210.25, 80.5), PR.Pes()]
    n = 0
    for t in range(300):
        regs = [[], []]
        for r in range(2):
            for _ in range(int(rng.integers(1, 6))):
                ql = int(rng.integers(30, 100))
                regs[r].append(PR.Reg(**{k: v for k, v in reg(int(rng.integers(100, 1500)) + (L0 if rng.random() < .2 else 0), bool(rng.random() < .5), 0, ql, int(rng.integers(30, ql + 1))).items()
                                         if k in ("rb", "re", "qb", "qe", "rid", "score")}))
        got = PR.pair(o, regs[0], regs[1], pes, t * 7919, L_PAC, CTG_OFF)
        assert got == PR.pair_brute(o, regs[0], regs[1], pes, t * 7919, L_PAC, CTG_OFF), t
        n += got[0] > 0
    assert n > 100


def _pestat_pairs(inserts, orient=1, p0=1000, step=0):
    """one pair per insert size in the given orientation (0 FF, 1 FR, 2 RF, 3 RR), single full-length hits"""
    pairs = []
    for j, d in enumerate(inserts):
        q0 = p0 + (j * step) % 20000
        if orient == 1:
            pairs.append(([reg(q0, False, 0, 100, 100)], [fr_mate(q0, d)]))
        elif orient == 0:
            pairs.append(([reg(q0, False, 0, 100, 100)], [reg(q0 + d, False, 0, 100, 100)]))
        elif orient == 3:
            pairs.append(([reg(q0 + d, False, 0, 100, 100)], [reg(q0, False, 0, 100, 100)]))
        else:
            pairs.append(([reg(q0 + d, False, 0, 100, 100)], [fr_mate(q0, 0)]))
    return pairs


def _ref_pestat(pairs, **optkw):
    off, regs = arrays(pairs)
    lists = [PR.regs_from(regs[off[r]:off[r + 1]]) for r in range(len(off) - 1)]
    return PR.pestat(lists, PR.opt_from(None, **optkw), L_PAC)


def test_reference_pestat_obvious_quartiles():
    # 100, 101, ..., 199: n = 100, p25 = L[25] = 125, p75 = L[75] = 175, IQR 50: fences 25 .. 275 hold everything: avg 149.5, var (100^2 - 1) / 12
    pes = _ref_pestat(_pestat_pairs(range(100, 200)))
    assert [p.failed for p in pes] == [1, 0, 1, 1]
    assert pes[1].avg == F(299, 2) and abs(float(pes[1].std) - (9999 / 12) ** .5) < 1e-12
    # low = (int)(125 - 150 + .499) = -24 -> avg - 4 std = 34.03 is larger, so low stays; clamp to 1.  high = 175 + 150 = 325 > avg + 4 std = 264.96
    assert (pes[1].low, pes[1].high) == (1, 325)
    # ten equal values and an outlier: the 2-IQR fence (IQR 0) drops the outlier from the mean
    pes = _ref_pestat(_pestat_pairs([300] * 10 + [900]))
    assert pes[1].avg == 300 and pes[1].std == 0 and (pes[1].low, pes[1].high) == (300, 300)
    # the other orientations are told apart
    for o in range(4):
        pes = _ref_pestat(_pestat_pairs(range(200, 230), orient=o))
        assert [p.failed for p in pes] == [int(d != o) for d in range(4)], o


# ------------------------------------------------------------------------------------------------------------------------------
# pestat: the oracle and the library against the reference
# ------------------------------------------------------------------------------------------------------------------------------
def pestat_cases():
    """(name, aim, pairs, pair_batch, n_batches)"""
    rng = np.random.default_rng(21)
    normal = lambda n, m, s: [max(1, int(x)) for x in rng.normal(m, s, size=n)]
    cases = []
    cases.append(("nine_ten", "9 and 10 candidates: MIN_DIR_CNT", _pestat_pairs(normal(9, 400, 40), 1) + _pestat_pairs(normal(10, 300, 30), 0, p0=3000), None, 1))
    big = _pestat_pairs(normal(210, 400, 50), 1, step=61)
    cases.append(("five_percent", "an orientation just below (10 of 210 = 4.8 %) and just above (11 = 5.2 %) 5 % of the largest",
                  big + _pestat_pairs(normal(10, 300, 20), 0, p0=3000) + _pestat_pairs(normal(11, 300, 20), 3, p0=6000), None, 1))
    cases.append(("max_ins", "an insert size at max_ins and one beyond", _pestat_pairs(normal(40, 9000, 300) + [10000] * 3 + [10001] * 30, 1, step=0), None, 1))
    three = _pestat_pairs(normal(60, 300, 30) + normal(60, 500, 60) + normal(60, 800, 150), 1, step=97)
    cases.append(("three_batches", "a call split in three by pair_batch, the batches interleaved", three, [(j * 7) % 3 for j in range(180)], 3))
    skew = [max(1, int(x)) for x in rng.gamma(2.0, 120.0, size=300)]
    cases.append(("skewed", "a skewed distribution: the fences cut one tail", _pestat_pairs(skew, 1, step=53), None, 1))
    cases.append(("two_peaks", "two peaks: the quartiles fall in different peaks", _pestat_pairs(normal(150, 250, 20) + normal(150, 700, 40), 1, step=53), None, 1))
    cases.append(("low_clamped", "small insert sizes and a wide spread: low clamps to 1", _pestat_pairs([max(1, int(x)) for x in rng.normal(60, 45, size=200)], 1, step=53), None, 1))
    # candidate selection: a second hit at exactly 0.8 of the best votes, one point above does not; hits on different contigs do not
    sel = _pestat_pairs(normal(30, 400, 30), 1, step=131)
    for j, (a, b) in enumerate(sel):
        if j % 3 == 0:
            a.append(reg(20000 + j, False, 0, 100, 80))
        elif j % 3 == 1:
            b.append(reg(20000 + j, False, 10, 100, 81))
    sel.append(([reg(500, False, 0, 100, 100)], [fr_mate(L0 + 500, 300)]))
    sel.append(([reg(700, False, 0, 100, 100)], []))
    cases.append(("selection", "cal_sub at 0.8 of the best score and one above; different contigs; an unaligned end", sel, None, 1))
    return cases


_PESTAT = {}


def pestat_reference(name):
    """per case: per batch the four models of the reference and the count of insert sizes inside the 2-IQR fences is recomputed by the comparison"""
    if not _PESTAT:
        for c in pestat_cases():
            _PESTAT[c[0]] = c
    c = _PESTAT[name]
    if len(c) == 5:
        nm, aim, pairs, pb, nb = c
        pb = np.zeros(len(pairs), dtype=np.int32) if pb is None else np.array(pb, dtype=np.int32)
        off, regs = arrays(pairs)
        sites, alts = PR.Sites(), []
        for b in range(nb):
            lists = []
            for p in np.nonzero(pb == b)[0]:
                lists += [PR.regs_from(regs[off[2 * p]:off[2 * p + 1]]), PR.regs_from(regs[off[2 * p + 1]:off[2 * p + 2]])]
            alts.append(PR.alternatives(lambda s: PR.pestat(lists, PR.opt_from(), L_PAC, s), sites))
        assert len(sites.near) * 1000 <= sites.n, (name, len(sites.near), sites.n)
        TALLY.add(sites)
        c = _PESTAT[name] = c + (off, regs, pb, alts)
    return c


def compare_pestat(got, alts, who):
    """got: 4 PESTAT_DT rows; alts: the reference's acceptable answers.  The bound on std is the module header's."""
    msg = None
    for ref in alts:
        ok = True
        for d in range(4):
            g, r = got[d], ref[d]
            avg, std = float(r.avg), float(r.std)          # the mean correctly rounded: what one division of an exact sum gives
            tol = ((r.n + 4) / 2 + (avg / std if std else 0) + 2) * 2.0 ** -53 * std
            if (int(g["low"]), int(g["high"]), int(g["failed"])) != (r.low, r.high, r.failed) or float(g["avg"]) != avg or abs(float(g["std"]) - std) > tol:
                ok = False
                msg = (who, "orientation", d, "got", got[d], "reference", (r.low, r.high, r.failed, avg, std), "std within", tol)
                break
        if ok:
            return
    raise AssertionError(msg)


PESTAT_NAMES = ["nine_ten", "five_percent", "max_ins", "three_batches", "skewed", "two_peaks", "low_clamped", "selection"]


def check_pestat_case(name, lib, world, oracle):
    nm, aim, pairs, _, nb, off, regs, pb, alts = pestat_reference(name)
    if name == "nine_ten":
        assert [p.failed for p in alts[0][0]] == [0, 1, 1, 1]
    if name == "five_percent":
        assert [p.failed for p in alts[0][0]] == [1, 0, 1, 0]
    if name == "low_clamped":
        assert alts[0][0][1].low == 1
    if oracle is not None:
        got = oracle.pestat(world.oidx, off, regs, pb, nb)
        for b in range(nb):
            compare_pestat(got[4 * b:4 * b + 4], alts[b], "the oracle, case %s (%s), batch %d" % (name, aim, b))
    got = lib.dbg_pestat(world.idx, lib.opt_init(), off, regs, pb, nb)
    for b in range(nb):
        compare_pestat(got[4 * b:4 * b + 4], alts[b], "ssg_dbg_pestat, case %s (%s), batch %d" % (name, aim, b))


def check_five_percent_exact(lib, world, oracle):
    """10 pairs of one orientation beside 200 of another: exactly a twentieth.  0.05 as a double is above 1 / 20, so in real numbers 10 < 200 * 0.05 and the
    orientation has failed; in binary64 the product rounds to 10.0 and it is kept -- upstream's arithmetic, and the oracle's and the host code's.  The reference
    must call the comparison a near site and offer both answers, and everybody under test must give the binary64 one."""
    rng = np.random.default_rng(22)
    pairs = _pestat_pairs([max(1, int(x)) for x in rng.normal(400, 50, size=200)], 1, step=61) + _pestat_pairs([max(1, int(x)) for x in rng.normal(300, 20, size=10)], 0, p0=3000)
    off, regs = arrays(pairs)
    lists = [PR.regs_from(regs[off[r]:off[r + 1]]) for r in range(len(off) - 1)]
    sites = PR.Sites()
    alts = PR.alternatives(lambda s: PR.pestat(lists, PR.opt_from(), L_PAC, s), sites)
    assert len(sites.near) == 1 and len(alts) == 2 and [a[0].failed for a in alts] == [1, 0] and alts[0][1].failed == alts[1][1].failed == 0
    pb = np.zeros(len(pairs), dtype=np.int32)
    for who, got in (("the oracle", oracle.pestat(world.oidx, off, regs, pb, 1) if oracle is not None else None), ("ssg_dbg_pestat", lib.dbg_pestat(world.idx, lib.opt_init(), off, regs, pb, 1))):
        if got is not None:
            compare_pestat(got[:4], alts[1:], who + ", an orientation at exactly 5 % of the largest")


def test_emu_five_percent_at_exactly_a_twentieth(emu_lib, oracle, tmp_path_factory):
    check_five_percent_exact(emu_lib, World.get(emu_lib, oracle, tmp_path_factory.mktemp("pairref")), oracle)


@pytest.mark.parametrize("name", PESTAT_NAMES)
def test_emu_pestat_against_reference(name, emu_lib, oracle, tmp_path_factory):
    check_pestat_case(name, emu_lib, World.get(emu_lib, oracle, tmp_path_factory.mktemp("pairref")), oracle)


# ------------------------------------------------------------------------------------------------------------------------------
# primary marking, pairing, MAPQ, record selection: the oracle and the library's forms against the reference
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GROUP_NAMES)
def test_oracle_pair_final_against_reference(name, emu_lib, oracle, tmp_path_factory):
    run_oracle(oracle, World.get(emu_lib, oracle, tmp_path_factory.mktemp("pairref")), groups()[name])


@pytest.mark.parametrize("name", GROUP_NAMES)
def test_emu_pair_final_against_reference(name, emu_lib, oracle, tmp_path_factory, monkeypatch):
    g = groups()[name]
    outcome = run_library(emu_lib, World.get(emu_lib, oracle, tmp_path_factory.mktemp("pairref")), g, monkeypatch, "the emulation build")
    if name.startswith("q_1024"):
        # the lane forms answer, the wave form -- which takes the pairs of more than 16 regions -- refuses (error code 6)
        assert outcome == {"default": "overflow", "lds_off": "overflow", "wave": "overflow", "lane_global": "ok"} or all(v == "ok" for v in outcome.values()), outcome


def test_emu_negative_wave_threshold_means_zero(emu_lib, oracle, tmp_path_factory, monkeypatch):
    """SSG_PAIR_WAVE_MIN below 0 is taken as 0 (every pair with a region through the wave form): unclamped, the count of heavy pairs took in the padding lanes of
    its last wave and pairs were worked on twice"""
    g = groups()["form_boundaries"]
    w = World.get(emu_lib, oracle, tmp_path_factory.mktemp("pairref"))
    monkeypatch.setenv("SSG_PAIR_WAVE_MIN", "-5")
    monkeypatch.delenv("SSG_PAIR_LDS", raising=False)
    out, req_off, req = emu_lib.dbg_pair_final(w.idx, lib_opt(emu_lib, g), g.id0, g.off, g.regs, g.pes)
    compare(g, out, req_off, req, "the emulation build, SSG_PAIR_WAVE_MIN=-5")


def test_entry_points_refuse_malformed_lists(emu_lib, oracle, tmp_path_factory):
    """a bad list must not reach a kernel: offsets that go back, a contig that does not exist, an empty or overlong query interval, a position off the text"""
    w = World.get(emu_lib, oracle, tmp_path_factory.mktemp("pairref"))
    opt = emu_lib.opt_init()
    good = ([reg(1000, False, 0, 100, 100)], [fr_mate(1000, 400)])
    for field, value in (("rid", 2), ("rid", -1), ("qe", 0), ("qe", 311), ("rb", -5), ("re", 2 * L_PAC + 1), ("score", -1)):
        off, regs = arrays([good])
        regs[0][field] = value
        with pytest.raises(capi.SsgError, match="error -22"):
            emu_lib.dbg_pair_final(w.idx, opt, 0, off, regs, pes_array(FR))
        with pytest.raises(capi.SsgError, match="error -22"):
            emu_lib.dbg_pestat(w.idx, opt, off, regs, np.zeros(1, dtype=np.int32), 1)
    off, regs = arrays([good])
    off[1] = 3
    with pytest.raises(capi.SsgError, match="error -22"):
        emu_lib.dbg_pair_final(w.idx, opt, 0, off, regs, pes_array(FR))
    off, regs = arrays([good])
    with pytest.raises(capi.SsgError, match="error -22"):
        emu_lib.dbg_pestat(w.idx, opt, off, regs, np.array([1], dtype=np.int32), 1)
    bad_pes = pes_array(FR)
    bad_pes[1]["std"] = 0.0
    with pytest.raises(capi.SsgError, match="error -22"):
        emu_lib.dbg_pair_final(w.idx, opt, 0, off, regs, bad_pes)


# ------------------------------------------------------------------------------------------------------------------------------
# the product path without a test entry
# ------------------------------------------------------------------------------------------------------------------------------
SSG_F_NO_RESCUE = 0x20


def check_product_path(lib, prefix, n_pairs, read_len, seed, id0, who):
    """regions from align1_batch; mem_process_pairs without mate rescue, so that the stage's input is exactly those regions: ssg_pe_pes must be pestat(), the
    requests the reference's -- once with the model inferred, once with it given.  A request names its region by a slot of the pairing stage's own layout; a
    printed record also carries the region's index in its read (owner), so the read's first slot is reg - owner of any of its printed records, and an XA
    entry only exists next to the printed record it belongs to.  Returns (longest list, the sites the reference evaluated)."""
    kw = dict(ins_mean=800, ins_std=150) if read_len > 200 else {}
    _, seqs, seq, off = common.sim_reads(n_pairs, seed, read_len, fasta=prefix, **kw)
    idx = lib.index_load(prefix)
    opt = lib.opt_init()
    opt["flag"] |= SSG_F_NO_RESCUE
    reg_off, regs, _ = lib.align1_batch(idx, opt, seq, off)
    l_pac = int(lib.l.ssg_index_l_pac(idx))
    lens = [len(c[1]) if isinstance(c, tuple) else len(c) for c in common.simreads.read_fasta(prefix)]
    ctg_off = [0] + [int(x) for x in np.cumsum(lens)[:-1]]
    assert sum(lens) == l_pac
    ropt = PR.opt_from(opt[0])
    lists = [PR.regs_from(regs[reg_off[r]:reg_off[r + 1]]) for r in range(2 * n_pairs)]
    n_reg = np.diff(reg_off)
    sites = PR.Sites()
    pes_alts = PR.alternatives(lambda s: PR.pestat(lists, ropt, l_pac, s), sites)
    given = pes_array({1: (1, 2000, 523.25, 181.5)})

    def rows(req):
        base = {int(q["reg"]) - int(q["owner"]) for q in req if q["kind"] == PR.MAIN and q["reg"] >= 0}
        assert len(base) <= 1 and (base or all(q["reg"] < 0 for q in req)), req
        b = base.pop() if base else 0
        return [(int(q["kind"]), int(q["reg"]) - b if q["reg"] >= 0 else -1, int(q["owner"]), int(q["flag"]), int(q["mapq"])) for q in req]
    for label, pes0 in (("inferred", None), ("given", given)):
        res = capi.mem_process_pairs(lib, idx, opt, seq, off, id0=id0, pes0=pes0)
        if pes0 is None:
            compare_pestat(res.pes[:4], pes_alts, "%s: ssg_pe_pes, %d x 2x%d" % (who, n_pairs, read_len))
            assert [int(x) for x in res.pes["failed"][:4]] == [1, 0, 1, 1]
        rpes = [PR.Pes(int(p["low"]), int(p["high"]), int(p["failed"]), float(p["avg"]), float(p["std"])) for p in res.pes[:4]]
        s2 = PR.Sites()
        for p in range(n_pairs):
            alts = PR.alternatives(lambda s: PR.pair_final(ropt, lists[2 * p], lists[2 * p + 1], rpes, id0 + p, l_pac, ctg_off, s), s2)
            got = [rows(res.req[res.req_off[2 * p + i]:res.req_off[2 * p + i + 1]]) for i in range(2)]
            assert any(got == recs for _, recs in alts), "%s, model %s: the requests of pair %d (%d + %d regions) disagree with the pairing reference\n got  %s\n want %s" % (
                who, label, p, n_reg[2 * p], n_reg[2 * p + 1], got, alts[0][1])
        assert len(s2.near) * 1000 <= s2.n, (len(s2.near), s2.n)
        sites.add(s2)
        res.close()
    lib.index_destroy(idx)
    _record_margins(sites, "product_%d" % read_len)
    return int(n_reg.max())


def _record_margins(sites, tag):
    """at most 1 site in 1000 near; where SSG_PAIR_MARGINS_OUT names a directory, the figures go to <tag>.json there (profiles/pair_margins.json is put together
    from those files of an emulator run and of an MI355X run)"""
    rec = dict(sites=sites.n, near=len(sites.near), min_margin=sites.min_margin)
    assert rec["sites"] > 0 and rec["near"] * 1000 <= rec["sites"], (tag, rec)
    out = os.environ.get("SSG_PAIR_MARGINS_OUT")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, tag + ".json"), "w") as f:
            json.dump(rec, f)
    return rec


@pytest.mark.parametrize("read_len", [150, 250])
def test_emu_product_path_against_reference(read_len, emu_lib, repeat_pe_prefix):
    longest = check_product_path(emu_lib, repeat_pe_prefix, 750, read_len, seed=31 + read_len, id0=12345, who="the emulation build")
    assert longest >= 64, "the repeat-rich reference gives region lists for the wave form"


# ------------------------------------------------------------------------------------------------------------------------------
# GPU twins: the same lists through the HIP build -- the only tests that run the device's log and erfc
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", PESTAT_NAMES)
def test_gpu_pestat_against_reference(name, gpu_lib, tmp_path_factory):
    check_pestat_case(name, gpu_lib, World.get(gpu_lib, None, tmp_path_factory.mktemp("pairref")), None)


@pytest.mark.gpu
def test_gpu_five_percent_at_exactly_a_twentieth(gpu_lib, tmp_path_factory):
    check_five_percent_exact(gpu_lib, World.get(gpu_lib, None, tmp_path_factory.mktemp("pairref")), None)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GROUP_NAMES)
def test_gpu_pair_final_against_reference(name, gpu_lib, tmp_path_factory, monkeypatch):
    g = groups()[name]
    outcome = run_library(gpu_lib, World.get(gpu_lib, None, tmp_path_factory.mktemp("pairref")), g, monkeypatch, "the HIP build")
    if name.startswith("q_1024"):
        assert outcome == {"default": "overflow", "lds_off": "overflow", "wave": "overflow", "lane_global": "ok"} or all(v == "ok" for v in outcome.values()), outcome


@pytest.mark.gpu
@pytest.mark.parametrize("read_len", [150, 250])
def test_gpu_product_path_against_reference(read_len, gpu_lib, repeat_pe_prefix):
    check_product_path(gpu_lib, repeat_pe_prefix, 750, read_len, seed=31 + read_len, id0=12345, who="the HIP build")


def test_zz_near_sites_of_the_constructed_inputs():
    """Over every constructed input of this module -- all groups and all insert-size cases, evaluated here unless a test above has done so; the simulated reads of
    the product path keep a tally of their own -- how many truncation sites the reference met, how many were near, and the smallest margin.  The same figures
    whichever tests ran before."""
    for g in groups().values():
        g.reference()
    for name in PESTAT_NAMES:
        pestat_reference(name)
    rec = _record_margins(TALLY, "constructed")
    assert rec["sites"] > 100000 and rec["near"] == 0, rec
