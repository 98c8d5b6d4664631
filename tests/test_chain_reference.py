"""The chaining stage (mem_chain with test_and_merge, mem_chain_weight, mem_chain_flt, frac_rep) against tests/chain_reference.py.

Three legs.  (1) The reference against itself: hand-worked cases, a second floor search, explicit position sets, every order of small tie groups, the binary32
helper against numpy.  (2) Constructed seed lists, in groups that each name their aim and assert ON THE REFERENCE ALONE that the branch was reached, through the
oracle (orc_api_chain) and through the library's test entry (ssg_dbg_chain: the host function stage 1 of the pipeline runs) in every kernel form.  (3) The seeds
and intervals of simulated reads.  The comparisons run on the emulation build; the `gpu' twins of legs 2 and 3 run the HIP build.

Rule.  For a read without a shared position the chains that survive -- (pos, rid, seed indices), w, kept, frac_rep bit for bit, and their order -- equal the
reference's: the oracle and every library form are each held to it.  A read whose weights are all distinct is ordered by the reference itself; another takes the
order the oracle's sort left, which the reference validates.  Reads with a shared position are left to the oracle.  Library == oracle, word for word, holds for
every read."""
import json
import os
from fractions import Fraction as F
from itertools import permutations

import numpy as np
import pytest

import chain_reference as cr
import common
from speedseq_amd import capi

FORMS = [
    ("default", {}),
    ("lds_off", {"SSG_CHAIN_LDS": "0"}),
    ("wave8", {"SSG_CHAIN_WAVE_MIN": "8"}),
    ("wave8_shifting", {"SSG_CHAIN_WAVE_MIN": "8", "SSG_CHAIN_RANKED": "0"}),
    ("lane_all", {"SSG_CHAIN_WAVE_MIN": "100000"}),
    ("wave_big", {"SSG_CHAIN_WAVE_MIN": "8", "SSG_CHAIN_WAVE_BIG": "16"}),
    ("cap_test", {"SSG_CHAIN_WAVE_MIN": "8", "SSG_CHAIN_CAP_TEST": "4"}),
]
LANE, LDS16, LDS32, LDS64 = capi.CHAIN_FORM_LANE, capi.CHAIN_FORM_LDS16, capi.CHAIN_FORM_LDS32, capi.CHAIN_FORM_LDS64
W256, W512, W1024, W2048, W5120 = capi.CHAIN_FORM_WAVE256, capi.CHAIN_FORM_WAVE512, capi.CHAIN_FORM_WAVE1024, capi.CHAIN_FORM_WAVE2048, capi.CHAIN_FORM_WAVE5120
ALL_FORMS = {LANE, LDS16, LDS32, LDS64, W256, W512, W1024, W2048, W5120}
L_PAC = 4000000
NO_DROP = dict(drop_ratio=0.0, min_chain_weight=0, max_chain_extend=1 << 30)
PADS_LONG = (0, 20, 40, 70, 300, 600, 1100, 2100)     # seed counts a scenario is padded to: LDS 16 / 32 / 64, wave 256 .. 5120 under the default split
PADS_SHORT = (0, 20, 40, 70, 300)


def expected_form(ns, env, n_ctg):
    """the class split of the chaining stage as DESIGN.md and ssgpu_core.cpp document it: by seed count, under the SSG_CHAIN_* switches"""
    t = 1 << 30 if n_ctg > 32767 else max(1, int(env.get("SSG_CHAIN_WAVE_MIN", 48)))
    tb = int(env.get("SSG_CHAIN_WAVE_BIG", 0)) or 1 << 30
    if ns >= t:
        if ns > 5120:
            return LANE
        for cls, form in ((2048, W5120), (1024, W2048), (512, W1024), (256, W512)):
            if ns > min(cls, tb):
                return form
        return W256
    if env.get("SSG_CHAIN_LDS", "1") == "0" or n_ctg >= 0x3fff or ns > 63:
        return LANE
    return LDS64 if ns > 31 else LDS32 if ns > 15 else LDS16


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
class Rd:
    def __init__(self, rl, seeds, intv=(), tag="", expect=None, survivors=None, kept=None):
        self.rl, self.seeds, self.intv, self.tag = rl, [tuple(int(v) for v in s) for s in seeds], [tuple(i) for i in intv], tag
        self.expect, self.survivors, self.kept = expect or {}, survivors, kept     # conditions on the reference: info counters, #survivors, kept values in final order


def pad(rd, n, l_pac):
    """the same read with seeds upstream drops (rid < 0) in front and behind, up to n seeds: the class split goes by seed count, chaining skips them"""
    k = n - len(rd.seeds)
    if k <= 0:
        return rd
    fill = [((7919 * i + 13 * n) % (l_pac - 400), i % 50, 19 + i % 7, -1 - i % 3) for i in range(k)]
    fill = [(r, q, min(l, rd.rl - q), rid) for r, q, l, rid in fill if q < rd.rl]
    h = len(fill) // 2
    expect = {k: v for k, v in rd.expect.items() if k != "skipped"}
    return Rd(rd.rl, fill[:h] + rd.seeds + fill[h:], rd.intv, "%s+pad%d" % (rd.tag, n), expect, rd.survivors, rd.kept)


class Group:
    def __init__(self, name, aim, scenarios, opt=None, l_pac=L_PAC, n_ctg=3, shared=False, near=False, pads=True, forms=None):
        self.name, self.aim, self.opt, self.l_pac, self.n_ctg, self.shared, self.near = name, aim, dict(opt or {}), l_pac, n_ctg, shared, near
        self.reads = []
        for k, s in enumerate(scenarios):
            for n in ((PADS_LONG if k < 2 else PADS_SHORT) if pads else (0,)):
                p = pad(s, n, l_pac)
                if n == 0 or p is not s:
                    self.reads.append(p)
        self.forms = forms       # kernel forms that must have taken reads of this group over the runs of FORMS (None: all of them)
        self._ref = None

    def packed(self):
        read_len = np.array([r.rl for r in self.reads], dtype=np.int32)
        seed_off = np.zeros(len(self.reads) + 1, dtype=np.int64); seed_off[1:] = np.cumsum([len(r.seeds) for r in self.reads])
        intv_off = np.zeros(len(self.reads) + 1, dtype=np.int64); intv_off[1:] = np.cumsum([len(r.intv) for r in self.reads])
        s4 = np.array([s for r in self.reads for s in r.seeds], dtype=np.int64).reshape(-1, 4)
        seeds = np.zeros(len(s4), capi.SEED_DT)
        seeds["rbeg"], seeds["qbeg"], seeds["len"] = s4[:, 0], s4[:, 1], s4[:, 2]
        seeds["score"], seeds["next"] = 12345, 777      # (ignored by the entry)
        iv = [x for r in self.reads for x in r.intv]
        intv = np.zeros(len(iv), capi.INTV_DT)
        intv["info"] = np.array([(a << 32) | b for a, b, _ in iv], dtype=np.uint64)
        intv["x2"] = np.array([c for _, _, c in iv], dtype=np.uint64)
        return read_len, seed_off, s4, seeds, s4[:, 3].astype(np.int32), intv_off, intv

    def ropt(self):
        return cr.opt_from(**self.opt)

    def lib_opt(self, lib):
        o = lib.opt_init()
        for k, v in self.opt.items():
            o[k] = v
        return o

    def orc_opt(self, oracle):
        o = self.ropt()
        h = oracle.opt_chain(float(o["drop_ratio"]), float(o["mask_level"]), o["min_chain_weight"], o["max_chain_extend"], o["max_chain_gap"])
        return oracle.opt_chain2(h, o["w"], o["min_seed_len"], o["max_occ"])


def run_oracle(oracle, g):
    """per read: the chains after mem_chain_flt's sort, the dropped ones included, as (pos, rid, seed indices, w, kept, frac_rep bits)"""
    read_len, seed_off, s4, _, _, intv_off, intv = g.packed()
    off, rows, cs = oracle.chain(g.l_pac, read_len, seed_off, s4, intv_off, intv, opt=g.orc_opt(oracle))
    return [[(int(x[0]), int(x[1]), tuple(cs[int(x[6]):int(x[6]) + int(x[2])].tolist()), int(x[3]), int(x[4]), int(x[5])) for x in rows[off[r]:off[r + 1]]]
            for r in range(len(g.reads))]


def run_library(lib, g, env, monkeypatch):
    for k in ("SSG_CHAIN_LDS", "SSG_CHAIN_WAVE_MIN", "SSG_CHAIN_RANKED", "SSG_CHAIN_WAVE_BIG", "SSG_CHAIN_CAP_TEST", "SSG_CHAIN_KBTREE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    read_len, seed_off, _, seeds, rids, intv_off, intv = g.packed()
    off, ch, cs, form = lib.dbg_chain(g.lib_opt(lib), g.l_pac, g.n_ctg, read_len, seed_off, seeds, rids, intv_off, intv)
    bits = ch["frac_rep"].view(np.uint32)
    rows = [[(int(c["pos"]), int(c["rid"]), tuple(cs[c["first_seed"]:c["first_seed"] + c["n"]].tolist()), int(c["w"]), int(c["kept"]), int(b))
             for c, b in zip(ch[off[r]:off[r + 1]], bits[off[r]:off[r + 1]])] for r in range(len(g.reads))]
    return rows, form


def reference(g, orows, tally):
    """every read of the group through the reference; the oracle's rows give the order of the reads whose weights tie, and nothing else"""
    opt, out = g.ropt(), []
    for r, rd in enumerate(g.reads):
        def order_of(cl, ws, rows=orows[r]):
            key = {(c[0], c[1], tuple(c[2])): k for k, c in enumerate(cl)}
            return [key[x[:3]] for x in rows]
        t = cr.Tally()
        res = cr.read(opt, g.l_pac, rd.rl, rd.seeds, rd.intv, order_of=order_of, tally=t)
        if not res["shared_position"]:
            tally.add(t)
            res["sites"] = t
        out.append(res)
    return out


_REFS, TALLY, COUNTS = {}, cr.Tally(), {}


def group_reference(g, oracle):
    if g.name not in _REFS:
        orows = run_oracle(oracle, g)
        t = cr.Tally()
        refs = reference(g, orows, t)
        check_conditions(g, refs, t)
        if not g.near:
            TALLY.add(t)
        COUNTS[g.name] = dict(reads=len(refs), seeds=sum(len(r.seeds) for r in g.reads), tie_free=sum(1 for x in refs if x["tie_free"]),
                              shared_position=sum(1 for x in refs if x["shared_position"]), sites=t.n, near=len(t.near))
        _REFS[g.name] = (orows, refs)
    return _REFS[g.name]


def check_conditions(g, refs, t):
    """what the group claims, asserted on the reference alone before anything is compared"""
    n_shared = sum(1 for x in refs if x["shared_position"])
    if g.shared:
        assert n_shared > 0, (g.name, "the group built for shared positions has none")
    else:
        assert n_shared == 0, (g.name, [rd.tag for rd, x in zip(g.reads, refs) if x["shared_position"]])
        assert 2 * sum(1 for x in refs if x["tie_free"]) >= len(refs), (g.name, "fewer than half of the reads are tie-free")
    if g.near:
        assert t.near, (g.name, "no near site")
    else:
        assert len(t.near) * 1000 <= t.n or not t.near, (g.name, len(t.near), t.n)
    for rd, x in zip(g.reads, refs):
        for k, v in rd.expect.items():
            assert x["info"][k] == v, (g.name, rd.tag, k, x["info"])
        if x["shared_position"]:
            continue
        if rd.survivors is not None:
            assert len(x["survivors"]) == rd.survivors, (g.name, rd.tag, x["survivors"])
        if rd.kept is not None:
            assert [k for _, k in x["marks"]] == rd.kept, (g.name, rd.tag, x["marks"], x["weights"])


def hold_to_reference(rows, refs, g, who, full=False):
    """rows[r]: (pos, rid, seeds, w, kept, frac bits) of read r in the order under test (full: the oracle's list with the dropped chains)"""
    n = 0
    for r, (got, x) in enumerate(zip(rows, refs)):
        if x["shared_position"]:
            continue
        ctx = (who, g.name, g.reads[r].tag, r)
        assert [c[:5] for c in got if c[4]] == x["survivors"], ctx
        assert all(c[5] == x["frac_rep_bits"] for c in got), ctx
        if full:
            cl = x["chains"]
            assert [c[:5] for c in got] == [(cl[i][0], cl[i][1], tuple(cl[i][2]), x["weights"][i], k) for i, k in x["marks"]], ctx
        n += 1
    return n


def check_group(g, lib, oracle, monkeypatch, who):
    orows, refs = group_reference(g, oracle)
    hold_to_reference(orows, refs, g, "the oracle", full=True)
    seen = set()
    for tag, env in FORMS:
        rows, form = run_library(lib, g, env, monkeypatch)
        assert [int(f) & 15 for f in form] == [expected_form(len(rd.seeds), env, g.n_ctg) for rd in g.reads], (who, g.name, tag)
        for r, x in enumerate(refs):
            if int(form[r]) & capi.CHAIN_FORM_TREE:     # the second pass is for reads with more than 9 chains and two at one position
                assert x["shared_position"] and len(x["chains"]) > 9, (who, g.name, tag, r)
        hold_to_reference(rows, refs, g, "%s, %s" % (who, tag))
        assert rows == [[c for c in o if c[4]] for o in orows], (who, g.name, tag)      # library == oracle, every read
        seen |= {int(f) & 15 for f in form}
        COUNTS[g.name]["reads_per_form_" + tag] = {str(k): int(sum(1 for f in form if int(f) == k)) for k in sorted({int(f) for f in form})}
        if g.shared:
            assert any(int(f) & capi.CHAIN_FORM_TREE for f in form), (who, g.name, tag, "no read went to the tree pass")
    want = ALL_FORMS if g.forms is None else g.forms
    assert want <= seen, (who, g.name, sorted(want - seen))


# ------------------------------------------------------------------------------------------------------------------------------
# the groups
# ------------------------------------------------------------------------------------------------------------------------------
def _two(first, second, rl=310, **kw):
    return Rd(rl, [first + (0,) if len(first) == 3 else first, second + (0,) if len(second) == 3 else second], **kw)


def g_merge_limits():
    """test_and_merge's inequalities at their limits, w = 100, max_chain_gap = 50 (reads end at 310)"""
    A = (100000, 100, 20)
    sc = []
    ok, no = dict(appended=1, new=1), dict(appended=0, new=2, refused_band=1)
    # x - y = w and w + 1 (y = 0 in the first: the seed sits at the chain's own position); y - x = w and w + 1 need a gap limit above them
    sc.append(_two(A, (100000 + 30, 160, 21), tag="x=60,y=30,gaps 40/10: in", expect=ok))
    sc.append(_two(A, (100000 + 69, 169, 22), tag="x-len=49,y-len=49: in", expect=ok))
    sc.append(_two(A, (100000 + 69, 170, 22), tag="x-len=50: out", expect=no))
    sc.append(_two(A, (100000 + 70, 169, 22), tag="y-len=50: out", expect=no))
    sc.append(_two((100000, 100, 60), (100000, 200, 21), tag="x-y=w, y=0: in", expect=ok))
    sc.append(_two((100000, 100, 60), (100001, 202, 21), tag="x-y=w+1 (y=1): out", expect=no))
    sc.append(_two((100000, 100, 60), (100000 + 100, 100, 21), tag="y-x=w: in", expect=ok))
    sc.append(_two((100000, 100, 60), (100000 + 101, 100, 21), tag="y-x=w+1: out", expect=no))
    # y = -1 against the LAST seed of the floor chain (the seed is still at or above the chain's position)
    sc.append(Rd(310, [(100000, 100, 20, 0), (100040, 140, 20, 0), (100039, 150, 30, 0)], tag="y=-1: out", expect=dict(appended=1, new=2, refused_band=1)))
    sc.append(Rd(310, [(100000, 100, 20, 0), (100040, 140, 20, 0), (100040, 150, 30, 0)], tag="y=0 against the last: in", expect=dict(appended=2, new=1)))
    # contained: accepted, n unchanged; contained on the query but not on the reference: judged by the band instead
    sc.append(Rd(310, [(100000, 100, 20, 0), (100040, 140, 30, 0), (100010, 110, 25, 0)], tag="contained", expect=dict(appended=1, contained=1, new=1)))
    sc.append(Rd(310, [(100000, 100, 20, 0), (100040, 140, 30, 0), (100120, 110, 25, 0)], tag="contained on the query only, off the band", expect=dict(appended=1, contained=0, new=2, refused_band=1)))
    sc.append(Rd(310, [(100000, 100, 20, 0), (100040, 140, 30, 0), (100050, 112, 21, 0)], tag="query inside, reference beyond, in the band", expect=dict(appended=2, contained=0, new=1)))
    # the floor chain refuses while an earlier chain would accept: only the floor is tried
    sc.append(Rd(310, [(100000, 100, 20, 0), (100300, 10, 23, 0), (100330, 130, 24, 0)], tag="floor refuses, earlier would take it", expect=dict(new=3, refused_band=2)))
    sc.append(Rd(310, [(100000, 100, 20, 0), (99000, 100, 21, 0), (98000, 100, 22, 0)], tag="below every position", expect=dict(new=3, below_all=2)))
    return Group("merge_limits", g_merge_limits.__doc__, sc, opt=dict(max_chain_gap=50, w=100, **NO_DROP))


def g_strands_contigs():
    """forward / reverse strand, contigs, dropped seeds, the 14-bit contig field of the LDS kernel"""
    lp = L_PAC
    sc = [
        Rd(310, [(lp - 40, 100, 20, 2), (lp + 10, 150, 21, 2)], tag="forward chain, seed at >= l_pac inside the band", expect=dict(new=2, refused_strand=1)),
        Rd(310, [(lp - 20, 100, 20, 2), (lp + 10, 130, 21, 2), (lp + 40, 160, 22, 2)], tag="chain whose seed ends at l_pac, then the reverse strand",
           expect=dict(new=2, refused_strand=1, appended=1)),
        Rd(310, [(lp + 10, 100, 20, 2), (lp + 40, 130, 21, 2)], tag="both on the reverse strand", expect=dict(new=1, appended=1)),
        Rd(310, [(500000, 100, 20, 0), (500030, 130, 21, 1)], tag="neighbouring contig inside the band", expect=dict(new=2, refused_contig=1)),
        Rd(310, [(500000, 100, 20, -1), (500030, 130, 21, 1), (500060, 160, 22, 1)], tag="dropped seed first", expect=dict(new=1, appended=1, skipped=1)),
        Rd(310, [(500000, 100, 20, 1), (500030, 130, 21, -2), (500060, 160, 22, 1)], tag="dropped seed in the middle", expect=dict(new=1, appended=1, skipped=1)),
        Rd(310, [(500000, 100, 20, -1), (500030, 130, 21, -1)], tag="every seed dropped", expect=dict(new=0, skipped=2), survivors=0),
        Rd(150, [], tag="no seeds", survivors=0),
    ]
    return Group("strands_contigs", g_strands_contigs.__doc__, sc, opt=dict(NO_DROP))


def _contig_group(name, n_ctg, forms):
    top = n_ctg - 1
    sc = [Rd(310, [(500000, 100, 20, top), (500030, 130, 21, top), (500060, 160, 22, top - 1)], tag="rid %d of %d" % (top, n_ctg), expect=dict(new=2, appended=1, refused_contig=1)),
          Rd(310, [(600000, 100, 25, 0), (600030, 130, 26, top)], tag="rid 0 and the top", expect=dict(new=2, refused_contig=1))]
    return Group(name, "contig ids at the width of the kernels' fields: n_ctg = %d" % n_ctg, sc, opt=dict(NO_DROP), n_ctg=n_ctg, forms=forms)


def g_ctg_3ffe():
    return _contig_group("n_ctg_0x3ffe", 0x3ffe, None)


def g_ctg_3fff():
    return _contig_group("n_ctg_0x3fff", 0x3fff, ALL_FORMS - {LDS16, LDS32, LDS64})     # no room for "none" in 14 bits: the global lane kernel


def g_ctg_4000():
    return _contig_group("n_ctg_0x4000", 0x4000, ALL_FORMS - {LDS16, LDS32, LDS64})


def g_ctg_32767():
    return _contig_group("n_ctg_32767", 32767, ALL_FORMS - {LDS16, LDS32, LDS64})


def g_ctg_32768():
    return _contig_group("n_ctg_32768", 32768, {LANE})          # beyond the wave kernels' 16-bit contigs: everything on the global lane kernel


def g_big_l_pac():
    """l_pac near 3.1e9: positions beyond 2^32, pairs of rbeg equal in the low 32 bits"""
    lp = 3100000000
    lo = 1500000000
    hi = lo + (1 << 32)           # the same low word, on the reverse strand (< 2 l_pac)
    sc = [
        Rd(310, [(lo, 100, 20, 0), (hi, 100, 21, 0), (lo + 30, 130, 22, 0), (hi + 30, 130, 23, 0)], tag="two chains equal in the low 32 bits", expect=dict(new=2, appended=2)),
        Rd(310, [(hi, 100, 20, 0), (lo, 100, 21, 0), (hi + 30, 130, 24, 0), (lo + 30, 130, 23, 0)], tag="the same, upper first", expect=dict(new=2, appended=2)),
        Rd(310, [(2 * lp - 60, 100, 20, 1), (2 * lp - 25, 135, 25, 1)], tag="a seed that ends at 2 l_pac", expect=dict(new=1, appended=1)),
        Rd(310, [((1 << 32) - 10, 100, 20, 1), ((1 << 32) + 20, 130, 21, 1)], tag="a chain across 2^32", expect=dict(new=1, appended=1)),
    ]
    return Group("big_l_pac", g_big_l_pac.__doc__, sc, opt=dict(NO_DROP), l_pac=lp)


def g_query_coordinates():
    """query coordinates at and beyond 256: the ninth bit of fq / lq / ll in the wave kernels, the 9-bit fields of the LDS kernel"""
    sc = []
    for rl in (255, 256, 257, 310):
        sc.append(Rd(rl, [(200000, rl - 60, 20, 0), (200035, rl - 25, 25, 0), (700000, 0, rl, 0)], tag="read of %d: last seed ends at the read's end, a seed of the whole read" % rl,
                     expect=dict(new=2, appended=1)))
    sc.append(Rd(310, [(300000, 200, 30, 0), (300060, 260, 31, 0), (300100, 280, 30, 0)], tag="first seed below 256, last at 256 or beyond", expect=dict(new=1, appended=2)))
    sc.append(Rd(310, [(300000, 270, 30, 0), (300010, 230, 31, 0), (300030, 200, 32, 0)], tag="first seed at 270, later seeds below 256 (negative x in the band)", expect=dict(new=1, appended=2)))
    sc.append(Rd(310, [(300000, 10, 256, 0), (300020, 40, 270, 0), (800000, 0, 300, 0)], tag="seeds of 256 bases and more", expect=dict(new=2, appended=1)))
    sc.append(Rd(310, [(300000, 255, 20, 0), (300001, 256, 21, 0), (300002, 257, 22, 0), (900000, 256, 54, 0)], tag="qbeg 255 / 256 / 257", expect=dict(new=2, appended=2)))
    return Group("query_coordinates", g_query_coordinates.__doc__, sc, opt=dict(mask_level=0.5, drop_ratio=0.5))


CLASS_COUNTS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
TOP_COUNTS = (2047, 2048, 2049)
TOP_COUNTS_5120 = (5119, 5120, 5121)
# a chain per seed at the top: the last count of a class, and below 5120 the first beyond it (the reference's chaining and filter are quadratic in the chains: seconds
# for a read of 5120; beyond 5120 the global lane kernel takes the read, which the forms without wave kernels run on the read of 5120 chains too)
TOP_COUNTS_A, TOP_COUNTS_5120_A = (2048, 2049), (5120,)


def _one_chain_per_seed(n, salt):
    """n seeds, each a chain of its own (chains = capacity): 700 apart on the reference, visited in a scattered order; distinct lengths (= weights) while the
    read has room for them; beyond that, seeds of 1 to 3 bases on a grid of query positions 3 apart, so that only chains at one query position overlap"""
    order = [(k * 2654435761 + salt) % n for k in range(n)] if n > 1 else [0]
    if len(set(order)) != n:
        order = list(range(n))[::-1]
    seeds = []
    for k in order:
        if n <= 257:
            seeds.append((1000 + 700 * k, k % 7, 300 - k, 0))
        else:
            seeds.append((1000 + 700 * k, (k * 3) % 300, 1 + k % 3, 0))
    return Rd(310, seeds, tag="%d seeds, a chain each" % n, expect=dict(new=n))


def _few_chains(n, salt):
    """n seeds in three chains (fewer when n < 3) of distinct weights: every seed one base further on the reference than its chain's last"""
    nch = min(3, n)
    cnt, seeds = [0] * nch, []
    for k in range(n):
        c = (k * 7 + salt) % nch if k >= nch else k
        seeds.append((100000 + 1000000 * c + cnt[c], 20 * c + (cnt[c] % 2), 40 + 11 * c, 0))
        cnt[c] += 1
    return Rd(310, seeds, tag="%d seeds in %d chains" % (n, nch), expect=dict(new=nch, appended=n - nch, contained=0))


def g_class_boundaries():
    """reads with exactly the seed counts at which the class split changes kernels, in two shapes; no chain dropped, so mem_chain alone is observed"""
    sc = []
    for n in CLASS_COUNTS:
        sc.append(_one_chain_per_seed(n, 3))
        sc.append(_few_chains(n, 1))
    return Group("class_boundaries", g_class_boundaries.__doc__, sc, opt=dict(NO_DROP), pads=False, forms=ALL_FORMS - {W5120})


def g_class_boundaries_top():
    """the same at 2047 .. 2049 seeds"""
    sc = [_few_chains(n, 1) for n in TOP_COUNTS] + [_one_chain_per_seed(n, 3) for n in TOP_COUNTS_A]
    return Group("class_boundaries_top", g_class_boundaries_top.__doc__, sc, opt=dict(NO_DROP), pads=False, forms={LANE, W2048, W5120})


def g_class_boundaries_5120():
    """the same at 5119 .. 5121 seeds (beyond 5120: the global lane kernel)"""
    sc = [_few_chains(n, 1) for n in TOP_COUNTS_5120] + [_one_chain_per_seed(n, 3) for n in TOP_COUNTS_5120_A]
    return Group("class_boundaries_5120", g_class_boundaries_5120.__doc__, sc, opt=dict(NO_DROP), pads=False, forms={LANE, W5120})


def g_floor_beyond_4096():
    """Counter-example found by this reference: the shifting form of ssg_k_chain_wave<5120> looked up a seed's floor chain in two levels of 64 lanes, which
    reach 4096 chains; with more, a floor chain in the rest of its block was missed and the seed opened a chain of its own or met the wrong one.  A read of
    4700 seeds, a chain each, in every form that takes it (and one of as many seeds in three chains, which never went wrong)"""
    return Group("floor_beyond_4096", g_floor_beyond_4096.__doc__, [_one_chain_per_seed(4700, 5), _few_chains(4700, 2)], opt=dict(NO_DROP), pads=False, forms={LANE, W5120})


def _singles(spans, rl=310):
    """one-seed chains (query begin, length = weight), far apart on the reference, visited in the order given"""
    return [(100000 + 5000 * k, q, l, 0) for k, (q, l) in enumerate(spans)]


def g_filter():
    """mem_chain_flt's comparisons at their limits (mask_level = drop_ratio = 0.5, min_seed_len = 19)"""
    sc = [
        Rd(310, _singles([(0, 100), (80, 40)]), tag="overlap = min_l * mask_level: shadowed, revived as the first shadowed", kept=[3, 1]),
        Rd(310, _singles([(0, 100), (81, 40)]), tag="overlap one less", kept=[3, 3]),
        Rd(310, _singles([(0, 100), (10, 60), (50, 50)]), tag="w_i = w_j * drop_ratio: not below (the chain of 60 is the first shadowed one)", kept=[3, 1, 2]),
        Rd(310, _singles([(0, 100), (10, 60), (50, 49)]), tag="w_i one less: below", kept=[3, 1, 0]),
        Rd(310, _singles([(0, 100), (50, 49), (60, 30)]), tag="w_i below w_j * drop_ratio; the second shadowed chain stays dropped", kept=[3, 1, 0]),
        Rd(310, _singles([(0, 60), (35, 25), (10, 23), (0, 22)]), tag="w_j - w_i one less than 2 min_seed_len: stays; equal to it: dropped (25 is the first shadowed)", kept=[3, 1, 2, 0]),
        Rd(310, _singles([(0, 100), (10, 40), (20, 39), (200, 50), (210, 20)]), tag="kept 1, 2, 3 and 0 in one read", kept=[3, 3, 1, 0, 1]),
        Rd(310, _singles([(0, 19), (100, 18), (200, 30)]), tag="no overlap at all", kept=[3, 3, 3]),
    ]
    return Group("filter", g_filter.__doc__, sc)


def g_filter_gap():
    """min_l against max_chain_gap = 40: a shorter span of 40 is no large overlap, 39 is"""
    sc = [
        Rd(310, _singles([(0, 100), (10, 40)]), tag="min_l = max_chain_gap", kept=[3, 3]),
        Rd(310, _singles([(0, 100), (10, 39)]), tag="min_l one less", kept=[3, 1]),
    ]
    return Group("filter_gap", g_filter_gap.__doc__, sc, opt=dict(max_chain_gap=40))


def _extend_group(n):
    sc = [
        Rd(310, _singles([(0, 100), (5, 90), (10, 80), (15, 70), (200, 60)]), tag="four overlapping chains and one apart"),
        Rd(310, _singles([(0, 100), (10, 40), (20, 39), (200, 50), (210, 20)]), tag="kept 1 and 0 before the cut"),
    ]
    return Group("max_chain_extend_%d" % n, "the max_chain_extend cut at %d" % n, sc, opt=dict(max_chain_extend=n))


def g_min_weight():
    """min_chain_weight = 30: a chain of 29 goes, of 30 stays; every chain below it: no chains at all"""
    sc = [
        Rd(310, _singles([(0, 29), (100, 30), (200, 31)]), tag="29 / 30 / 31", survivors=2),
        Rd(310, _singles([(0, 29), (100, 28), (200, 19)]), tag="all below", survivors=0),
    ]
    return Group("min_chain_weight", g_min_weight.__doc__, sc, opt=dict(min_chain_weight=30))


def _many_chains(n, nodrop):
    """n one-seed chains entering the filter (the wave kernels test 64 sorted chains at a time): weights 300, 299, ... while they are distinct"""
    spans = [((3 * k) % 9, 300 - k if k < 290 else 5 + k % 5) for k in range(n)]
    order = [(k * 37 + 5) % n for k in range(n)]
    if len(set(order)) != n:
        order = list(range(n))[::-1]
    return Rd(310, [(100000 + 5000 * k, spans[k][0], spans[k][1], 0) for k in order], tag="%d chains into the filter%s" % (n, ", none dropped" if nodrop else ""), expect=dict(new=n))


def g_filter_blocks():
    """63 / 64 / 65 / 128 / 129 chains entering the filter; with the default options most are dropped"""
    return Group("filter_blocks", g_filter_blocks.__doc__, [_many_chains(n, False) for n in (63, 64, 65, 128, 129)], pads=False, forms={LANE, W256, W5120})


def g_filter_blocks_kept():
    """the same with nothing dropped: 64 / 65 and more chains kept"""
    sc = [_many_chains(n, True) for n in (63, 64, 65, 128, 129)]
    for s, n in zip(sc, (63, 64, 65, 128, 129)):
        s.survivors = n
    return Group("filter_blocks_kept", g_filter_blocks_kept.__doc__, sc, opt=dict(NO_DROP), pads=False, forms={LANE, W256, W5120})


def _spread(wa, wb, wc):
    """a chain of weight wa in two seeds that spans [0, 100 + wa / 2), and two one-seed chains of weights wb and wc inside that span, apart from one another:
    both overlap the first largely, the one of wb is the first it shadows, so the one of wc shows what its own comparison decided"""
    return [(100000, 0, wa - wa // 2, 0), (100100, 100, wa // 2, 0), (200000, 30, wb, 0), (300000, 80, wc, 0)]


def g_near_sites():
    """float32 products that round onto the integer they are compared with: mask_level = 0.3f with min_l = 20 and overlap 6 (the exact product is above 6, the
    binary32 product is 6.0); drop_ratio = 0.8f with (w_j, w_i) = (25, 20) and (30, 24), min_seed_len = 2 so that the weight difference passes"""
    sc = [
        Rd(310, _singles([(0, 100), (50, 21), (94, 20)]), tag="overlap 6 of min_l 20 at 0.3f: a large overlap as C has it, so dropped; exactly, kept = 3", kept=[3, 1, 0]),
        Rd(310, _spread(25, 24, 20), tag="20 against 25 * 0.8f: not below as C has it; exactly, dropped", kept=[3, 1, 2]),
        Rd(310, _spread(30, 29, 24), tag="24 against 30 * 0.8f: likewise", kept=[3, 1, 2]),
        Rd(310, _spread(30, 29, 23), tag="23 against 30 * 0.8f: below either way", kept=[3, 1, 0]),
    ]
    return Group("near_sites", g_near_sites.__doc__, sc, opt=dict(mask_level=0.3, drop_ratio=0.8, min_seed_len=2), near=True)


def g_weights_frac_rep():
    """chain weights with non-monotone and overlapping seeds; frac_rep from nested, adjacent and disjoint intervals, x2 at max_occ and above, ratios binary32 cannot hold"""
    sc = [
        Rd(150, [(400000, 60, 30, 0), (400005, 50, 25, 0), (400030, 80, 30, 0), (600000, 0, 19, 0)], [(0, 50, 501), (10, 30, 900), (50, 60, 501), (100, 120, 500), (120, 140, 501)],
           tag="qbeg goes back inside a chain; nested, adjacent, disjoint; 80 / 150", expect=dict(new=2, appended=2)),
        Rd(150, [(400000, 10, 40, 0), (400020, 30, 40, 0), (400025, 35, 20, 0), (400070, 80, 30, 0)], [(0, 50, 501)], tag="overlapping seeds; 50 / 150", expect=dict(new=1, appended=2, contained=1)),
        Rd(151, [(400000, 10, 40, 0), (400050, 40, 40, 0)], [(0, 101, 501), (101, 130, 500)], tag="query overlaps more than the reference; 101 / 151", expect=dict(new=1, appended=1)),
        Rd(151, [(400000, 10, 40, 0), (400020, 60, 40, 0)], [(0, 101, 500), (101, 130, 500)], tag="reference overlaps more than the query; x2 = max_occ only: 0", expect=dict(new=1, appended=1)),
        Rd(310, [(400000, 0, 19, 0)], [(0, 1, 501), (1, 2, 501), (3, 310, 501)], tag="309 / 310"),
    ]
    return Group("weights_frac_rep", g_weights_frac_rep.__doc__, sc)


def g_shared_positions():
    """chains at one position, and more than nine chains: the answer depends on klib's container, so the reference flags the reads and they are compared with the oracle only"""
    sc = []
    for extra in (2, 12, 30):
        seeds = [(100000, 10, 25, 0), (100000, 200, 26, 0), (100000, 120, 24, 0)]            # three chains at one position (the band refuses each later one)
        seeds += [(200000 + 900 * k, 5 + k, 30 + k, 0) for k in range(extra)]
        seeds += [(100030, 40, 27, 0), (100000, 230, 28, 0), (200000 + 900 * 1, 150, 19, 0)]
        sc.append(Rd(310, seeds, tag="three chains at one position and %d others" % extra))
    return Group("shared_positions", g_shared_positions.__doc__, sc, opt=dict(NO_DROP), shared=True)


GROUPS = [g_merge_limits, g_strands_contigs, g_ctg_3ffe, g_ctg_3fff, g_ctg_4000, g_ctg_32767, g_ctg_32768, g_big_l_pac, g_query_coordinates, g_class_boundaries, g_class_boundaries_top, g_class_boundaries_5120, g_floor_beyond_4096,
          g_filter, g_filter_gap, lambda: _extend_group(1), lambda: _extend_group(2), lambda: _extend_group(3), g_min_weight, g_filter_blocks, g_filter_blocks_kept,
          g_near_sites, g_weights_frac_rep, g_shared_positions]
_GROUPS = {}


def groups():
    if not _GROUPS:
        for f in GROUPS:
            g = f()
            assert g.name not in _GROUPS
            _GROUPS[g.name] = g
    return _GROUPS


GROUP_NAMES = ["merge_limits", "strands_contigs", "n_ctg_0x3ffe", "n_ctg_0x3fff", "n_ctg_0x4000", "n_ctg_32767", "n_ctg_32768", "big_l_pac", "query_coordinates", "class_boundaries", "class_boundaries_top", "class_boundaries_5120", "floor_beyond_4096",
               "filter", "filter_gap", "max_chain_extend_1", "max_chain_extend_2", "max_chain_extend_3", "min_chain_weight", "filter_blocks", "filter_blocks_kept",
               "near_sites", "weights_frac_rep", "shared_positions"]


# ------------------------------------------------------------------------------------------------------------------------------
# leg 1: the reference against itself
# ------------------------------------------------------------------------------------------------------------------------------
def test_f32_against_numpy():
    rng = np.random.default_rng(7)
    vals = [F(1, 3), F(50, 150), F(101, 151), F(2, 3), F(1, 10), F(3, 10), F(16777217), F(16777219), F(1, 1 << 140), F(5, 1 << 149), F(3, 1 << 150), F(0)]
    vals += [F(int(a), int(b)) for a, b in zip(rng.integers(0, 311, 300), rng.integers(1, 311, 300))]
    for v in vals:
        want = np.float32(v.numerator) / np.float32(v.denominator) if v.denominator < (1 << 24) and v.numerator < (1 << 24) else np.float32(float(v))
        assert cr.f32(v) == F(float(want)), v
        assert cr.f32_bits(v) == int(np.array([want], dtype=np.float32).view(np.uint32)[0]), v
        assert cr.f32(-v) == -cr.f32(v)
    for c in (0.5, 0.3, 0.8, 0.7, 0.35):      # the option's binary32 value, and every product the filter can form with it
        c32 = cr.f32(F(c))
        assert c32 == F(float(np.float32(c)))
        for n in range(0, 311):
            assert cr.f32(n * c32) == F(float(np.float32(n) * np.float32(c))), (c, n)


def _near(c, lo=19, hi=310):
    """(n, m): integers m for which m >= n * c or m < n * c differ between the exact product and the binary32 product"""
    c32, out = cr.f32(F(c)), []
    for n in range(lo, hi + 1):
        exact, rounded = n * c32, cr.f32(n * c32)
        for m in {int(exact), int(exact) + 1, int(rounded), int(rounded) + 1}:
            if (m >= exact) != (m >= rounded) or (m < exact) != (m < rounded):
                out.append((n, m))
    return sorted(set(out))


def test_where_the_near_sites_are():
    assert (20, 6) in _near(0.3) and (25, 20) in _near(0.8) and (30, 24) in _near(0.8)
    assert _near(0.7) == [] and _near(0.35) == [] and _near(0.5) == []


def test_frac_rep_is_the_union_and_refuses_unsorted_input():
    o = cr.opt_from()
    assert cr.frac_rep(o, 150, [(0, 50, 501), (10, 30, 900), (50, 60, 501), (100, 120, 500), (120, 140, 501)]) == (80, cr.f32_bits(F(80, 150)))
    assert cr.frac_rep(o, 150, [(0, 50, 500)])[0] == 0 and cr.frac_rep(o, 150, [])[0] == 0
    assert cr.frac_rep(o, 151, [(0, 101, 501)])[1] == int(np.array([np.float32(101) / np.float32(151)]).view(np.uint32)[0])
    with pytest.raises(ValueError):
        cr.frac_rep(o, 150, [(10, 30, 501), (0, 50, 501)])


def test_hand_worked_chains():
    o = cr.opt_from()
    seeds = [(1000, 10, 20, 0), (1030, 40, 20, 0), (5000, 0, 19, 0), (1035, 45, 10, 0), (1031, 200, 20, 0), (900, 10, 20, 0), (1040, 50, 30, 1), (7, 7, 7, -1)]
    cl, shared, info = cr.chains(o, 10000, seeds)
    # seed 1 extends chain 0; 2 is far beyond the band of its floor (the chain at 1000); 3 is contained; 4 is off the band of its floor (the chain at 1000); 5 lies below everything;
    # 6 is on another contig than its floor (the chain at 1031); 7 is dropped
    assert cl == [(900, 0, [5]), (1000, 0, [0, 1]), (1031, 0, [4]), (1040, 1, [6]), (5000, 0, [2])] and not shared
    assert info == dict(contained=1, appended=1, refused_contig=1, refused_strand=0, refused_band=2, below_all=1, new=5, skipped=1)
    assert [cr.weight([seeds[i] for i in c[2]]) for c in cl] == [20, 40, 20, 30, 19]
    # a forward chain never takes a reverse-strand seed, whatever the band says
    cl, shared, info = cr.chains(o, 1040, [(1000, 10, 20, 0), (1040, 50, 20, 0)])
    assert len(cl) == 2 and info["refused_strand"] == 1
    # a second chain at a held position, and a look-up that lands on it: reported
    assert cr.chains(o, 10000, [(1000, 10, 20, 0), (1000, 200, 20, 0)])[1]
    assert not cr.chains(o, 10000, [(1000, 10, 20, 0), (1001, 200, 20, 0), (1002, 12, 20, 0)])[1]


def test_chains_against_a_second_floor_search():
    rng = np.random.default_rng(11)
    o = cr.opt_from(max_chain_gap=60)
    n_multi = 0
    for _ in range(200):
        seeds = []
        for _ in range(int(rng.integers(1, 40))):
            l = int(rng.integers(5, 40)); q = int(rng.integers(0, 150 - l))
            base = int(rng.choice([1000, 1400, 9000]))
            seeds.append((base + q + int(rng.integers(-120, 121)), q, l, int(rng.choice([0, 0, 0, 1, -1]))))
        cl, shared, _ = cr.chains(o, 9050, seeds)
        if shared:
            continue
        assert cl == cr.chains_brute(o, 9050, seeds)
        n_multi += any(len(c[2]) > 2 for c in cl)
    assert n_multi > 50


def test_weight_against_position_sets():
    rng = np.random.default_rng(12)
    for it in range(300):
        n = int(rng.integers(1, 8))
        sd = [(int(rng.integers(0, 200)), int(rng.integers(0, 100)), int(rng.integers(1, 40))) for _ in range(n)]
        if it % 2:           # begins that do not decrease on either axis: the weight is the measure of the union
            sd = sorted(sd, key=lambda s: s[0])
            qs = sorted(s[1] for s in sd)
            sd = [(s[0], q, s[2]) for s, q in zip(sd, qs)]
        w, per_axis, unions = cr.weight_sets(sd)
        assert cr.weight(sd) == w
        assert per_axis[0] <= unions[0] and per_axis[1] <= unions[1]
        if it % 2:
            assert per_axis == unions
    assert cr.weight([(0, 0, 1 << 31)]) == (1 << 30) - 1


def test_flt_hand_worked_and_tie_groups_under_every_order():
    o = cr.opt_from()
    seeds = _singles([(0, 100), (10, 40), (20, 39), (200, 50), (210, 20)])
    cl, _, _ = cr.chains(o, L_PAC, seeds)
    ws = [cr.weight([seeds[i] for i in c[2]]) for c in cl]
    # 100 keeps; 50 (apart) keeps; 40 is inside 100 and below half of it: dropped, but it is the first chain 100 shadows: kept = 1; 39 likewise dropped and stays so;
    # 20 is inside 50, below half, but 50 - 20 < 38: not dropped, and it is the first chain 50 shadows: kept = 1
    assert cr.flt(o, seeds, cl, ws) == [(0, 3), (3, 3), (1, 1), (2, 0), (4, 1)]
    assert cr.flt(cr.opt_from(min_chain_weight=101), seeds, cl, ws) == []
    with pytest.raises(ValueError):
        cr.flt(o, seeds, cl, ws, order=[0, 3, 2, 1])             # not a permutation
    with pytest.raises(ValueError):
        cr.flt(o, seeds, cl, ws, order=[3, 0, 1, 2, 4])          # weights increase
    # a tie group: four chains of weight 40 under one of 100, in every order the sort may leave them: the first of them is the one revived
    seeds = _singles([(0, 100), (10, 40), (20, 40), (30, 40), (40, 40)])
    cl, _, _ = cr.chains(o, L_PAC, seeds)
    ws = [cr.weight([seeds[i] for i in c[2]]) for c in cl]
    assert not cr.tie_free(o, ws)
    with pytest.raises(ValueError):
        cr.flt(o, seeds, cl, ws)
    for p in permutations([1, 2, 3, 4]):
        assert cr.flt(o, seeds, cl, ws, order=[0] + list(p)) == [(0, 3), (p[0], 1), (p[1], 0), (p[2], 0), (p[3], 0)]


def test_validation_of_the_entry(emu_lib):
    g = Group("v", "", [Rd(150, [(1000, 10, 20, 0), (1030, 40, 20, 0)], [(0, 30, 501), (10, 50, 3)])], pads=False)
    read_len, seed_off, _, seeds, rids, intv_off, intv = g.packed()
    ok = lambda **kw: emu_lib.dbg_chain(emu_lib.opt_init(), kw.get("l_pac", 5000), kw.get("n_ctg", 1), kw.get("read_len", read_len), kw.get("seed_off", seed_off),
                                        kw.get("seeds", seeds), kw.get("rids", rids), intv_off, kw.get("intv", intv))
    ok()

    def changed(a, f, v, k=0):
        b = a.copy()
        if f is None:
            b[k] = v
        else:
            b[f][k] = v
        return b
    bad = [dict(read_len=np.array([0], np.int32)), dict(read_len=np.array([311], np.int32)), dict(seed_off=np.array([0, 3], np.int64)[::-1].copy()),
           dict(seeds=changed(seeds, "qbeg", -1)), dict(seeds=changed(seeds, "len", 0)), dict(seeds=changed(seeds, "qbeg", 131)), dict(seeds=changed(seeds, "rbeg", -1)),
           dict(seeds=changed(seeds, "rbeg", 10000 - 19)), dict(rids=changed(rids, None, 1)), dict(intv=intv[::-1].copy()), dict(l_pac=0), dict(n_ctg=0)]
    for kw in bad:
        with pytest.raises(capi.SsgError, match="-22"):
            ok(**kw)


# ------------------------------------------------------------------------------------------------------------------------------
# leg 2: constructed seed lists
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GROUP_NAMES)
def test_emu_group_against_reference(name, emu_lib, oracle, monkeypatch):
    check_group(groups()[name], emu_lib, oracle, monkeypatch, "the emulation build")


@pytest.mark.gpu
@pytest.mark.parametrize("name", GROUP_NAMES)
def test_gpu_group_against_reference(name, gpu_lib, oracle, monkeypatch):
    check_group(groups()[name], gpu_lib, oracle, monkeypatch, "the HIP build")


# ------------------------------------------------------------------------------------------------------------------------------
# leg 3: the seeds and intervals of simulated reads
# ------------------------------------------------------------------------------------------------------------------------------
_REAL = {}


def realistic_group(oracle, prefix, tag, n_pairs, seed):
    """simulated reads of a reference: seeds and intervals from the oracle (seeds, collect_intv), as a Group"""
    if tag not in _REAL:
        oidx = oracle.idx_load(prefix)
        _, seqs, seq, off = common.sim_reads(n_pairs, seed, 150, fasta=prefix)
        sc = []
        for r, s in enumerate(seqs):
            sd = oracle.seeds(oidx, s)
            iv = oracle.collect_intv(oidx, s)
            sc.append(Rd(len(s), [tuple(x) for x in sd.tolist()], [(int(i["info"]) >> 32, int(i["info"]) & 0xffffffff, int(i["x2"])) for i in iv], tag="%s read %d" % (tag, r)))
        _REAL[tag] = (sc, seq, off, seqs)
    return _REAL[tag]


def check_realistic(lib, oracle, prefix, tag, n_pairs, seed, monkeypatch, who):
    sc, seq, off, seqs = realistic_group(oracle, prefix, tag, n_pairs, seed)
    idx = lib.index_load(prefix)
    lib.l.ssg_index_n_ctg.argtypes = [type(idx)]
    l_pac, n_ctg = int(lib.l.ssg_index_l_pac(idx)), int(lib.l.ssg_index_n_ctg(idx))
    g = Group(tag, "simulated reads", sc, l_pac=l_pac, n_ctg=n_ctg, pads=False, forms=set())
    g.shared = None
    # the entry's input is what the pipeline feeds its own chaining stage: the same seeds and intervals from the library's seeding stage
    read_len, seed_off, s4, seeds, rids, intv_off, intv = g.packed()
    for k in ("SSG_CHAIN_LDS", "SSG_CHAIN_WAVE_MIN", "SSG_CHAIN_RANKED", "SSG_CHAIN_WAVE_BIG", "SSG_CHAIN_CAP_TEST", "SSG_CHAIN_KBTREE"):
        monkeypatch.delenv(k, raising=False)
    so, sd, rd = lib.seeds_batch(idx, lib.opt_init(), seq, off)
    assert np.array_equal(so, seed_off) and np.array_equal(rd, rids), who
    for f in ("rbeg", "qbeg", "len"):
        assert np.array_equal(sd[f], seeds[f]), (who, f)
    cap = max(64, int(np.diff(intv_off).max()))
    li, ln = lib.smem_batch(idx, lib.opt_init(), seq, off, cap=cap)
    assert np.array_equal(ln, np.diff(intv_off)), who
    for r in range(len(sc)):
        for f in ("info", "x2"):
            assert np.array_equal(li[r, :ln[r]][f], intv[intv_off[r]:intv_off[r + 1]][f]), (who, r, f)
    lib.index_destroy(idx)
    # conditions on the reference alone
    if tag not in _REFS:
        orows = run_oracle(oracle, g)
        t = cr.Tally()
        refs = reference(g, orows, t)
        n_shared = sum(1 for x in refs if x["shared_position"])
        assert n_shared * 100 <= len(refs), (tag, n_shared, len(refs))
        assert len(t.near) * 1000 <= t.n, (tag, len(t.near), t.n)
        assert sum(len(x["chains"]) > 9 for x in refs) > 20, tag
        COUNTS[tag] = dict(reads=len(refs), seeds=sum(len(r.seeds) for r in g.reads), tie_free=sum(1 for x in refs if x["tie_free"]), shared_position=n_shared, sites=t.n, near=len(t.near))
        _REFS[tag] = (orows, refs)
    orows, refs = _REFS[tag]
    assert hold_to_reference(orows, refs, g, "the oracle", full=True) * 100 >= 99 * len(refs)
    for ftag, env in (FORMS[0], FORMS[2]):
        rows, form = run_library(lib, g, env, monkeypatch)
        assert [int(f) & 15 for f in form] == [expected_form(len(rd_.seeds), env, n_ctg) for rd_ in g.reads], (who, tag, ftag)
        hold_to_reference(rows, refs, g, "%s, %s" % (who, ftag))
        assert rows == [[c for c in o if c[4]] for o in orows], (who, tag, ftag)
        fc = COUNTS[tag].setdefault("reads_per_form_" + ftag, {})
        for f in form:
            fc[str(int(f))] = fc.get(str(int(f)), 0) + 1


def test_emu_slice_reads_against_reference(emu_lib, oracle, monkeypatch):
    check_realistic(emu_lib, oracle, common.EXAMPLE_FA, "slice", 300, 41, monkeypatch, "the emulation build")


def test_emu_repeat_mid_reads_against_reference(emu_lib, oracle, repeat_mid_prefix, monkeypatch):
    check_realistic(emu_lib, oracle, repeat_mid_prefix, "repeat_mid", 300, 42, monkeypatch, "the emulation build")


@pytest.mark.gpu
def test_gpu_slice_reads_against_reference(gpu_lib, oracle, monkeypatch):
    check_realistic(gpu_lib, oracle, common.EXAMPLE_FA, "slice", 300, 41, monkeypatch, "the HIP build")


@pytest.mark.gpu
def test_gpu_repeat_mid_reads_against_reference(gpu_lib, oracle, repeat_mid_prefix, monkeypatch):
    check_realistic(gpu_lib, oracle, repeat_mid_prefix, "repeat_mid", 300, 42, monkeypatch, "the HIP build")


def test_zz_what_the_reference_evaluated(oracle):
    """Over every constructed group -- evaluated here unless a test above has done so: reads, tie-free and shared-position shares, float comparison sites and near
    sites.  Outside the group built to sit on them no site is near.  Where SSG_CHAIN_COUNTS_OUT names a directory the figures go to chain_reference_counts.json
    there (profiles/chain_reference_counts.json is such a file)."""
    for g in groups().values():
        group_reference(g, oracle)
    assert TALLY.n > 20000 and not TALLY.near, (TALLY.n, TALLY.near[:5])
    n_reads = sum(COUNTS[n]["reads"] for n in GROUP_NAMES)
    assert 500 <= n_reads <= 10000 and sum(COUNTS[n]["seeds"] for n in GROUP_NAMES) >= 20000
    out = os.environ.get("SSG_CHAIN_COUNTS_OUT")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "chain_reference_counts.json"), "w") as f:
            json.dump(dict(constructed_sites=TALLY.n, constructed_near=len(TALLY.near), groups=COUNTS), f, indent=1, sort_keys=True)
