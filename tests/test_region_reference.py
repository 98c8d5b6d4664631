"""The region stage (mem_chain2aln per chain, then mem_sort_dedup_patch with mem_patch_reg) against tests/region_reference.py.

Three legs.  (1) The reference against itself: hand-worked chains, seedcov against position sets, the window against a per-base union, tie groups under every
order, the near sites located with numpy.float32.  (2) Constructed chains, in groups named after the boundaries of the device code (csrc/k_extend.h,
k_extlane.h, k_sdp.h, ssgpu_core.cpp run_regions); each group asserts ON THE REFERENCE ALONE that its boundary was reached (regions before the dedup, tallies),
then the oracle (orc_api_regions), the emulation build and -- `gpu' -- the HIP build (ssg_dbg_regions: the host function stage 1 of the pipeline runs) are each
held to the reference, every field, in order; route[] is asserted where a read is built for a route.  (3) The chains of simulated reads, and the composition
ssg_seeds_batch -> ssg_dbg_chain -> ssg_dbg_regions == ssg_align1_batch.

Rule.  A read the reference decides is compared with the reference by everyone.  A read the reference reports as order-dependent (unstable sorts, see
region_reference.py) is compared with the oracle only.  Library == oracle holds for every read."""
import json
import os
from fractions import Fraction as F

import numpy as np
import pytest

import common
import region_reference as rr
from speedseq_amd import capi

WAVE, PATCH = capi.REG_ROUTE_WAVE, capi.REG_ROUTE_PATCH
EINVAL, EOVERFLOW = -22, -75


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
def pac_of(text):
    l = len(text)
    c = np.zeros((l // 4 + 1) * 4, dtype=np.uint8)
    c[:l] = text
    c = c.reshape(-1, 4)
    return (c[:, 0] << 6 | c[:, 1] << 4 | c[:, 2] << 2 | c[:, 3]).astype(np.uint8)


def rc(codes):
    return [3 - int(c) for c in reversed(codes)]


class World:
    """a reference: forward codes, contigs that tile it"""

    def __init__(self, text, ctg_len=None, pac=None, l_pac=None):
        self.text = text
        self.l_pac = int(l_pac if l_pac is not None else len(text))
        self.pac = pac if pac is not None else pac_of(text)
        self.ctg_len = list(ctg_len or [self.l_pac])
        assert sum(self.ctg_len) == self.l_pac
        self.ctg_off = [int(x) for x in np.concatenate([[0], np.cumsum(self.ctg_len)[:-1]])]
        self.ref = rr.Ref(self.pac, self.l_pac, self.ctg_off, self.ctg_len)

    def fw(self, p, n):
        return [self.ref.base(k) for k in range(p, p + n)]     # doubled coordinates: p >= l_pac reads the reverse strand


_WORLDS = {}


def world(name):
    if name not in _WORLDS:
        if name == "two":
            _WORLDS[name] = World(np.random.RandomState(1).randint(0, 4, 200000).astype(np.uint8), [120000, 80000])
        elif name == "wide":          # rb may differ by 2^26: 2^26 + 2^17 bases
            _WORLDS[name] = World(np.random.RandomState(2).randint(0, 4, (1 << 26) + (1 << 17)).astype(np.uint8))
        elif name == "high":          # l_pac just above 2^31: the pac (513 MiB) made by tiling a random block of 4096 bases; no text is kept
            block = pac_of(np.random.RandomState(4).randint(0, 4, 4096).astype(np.uint8))[:1024]
            l_pac = (1 << 31) + 8192
            pac = np.concatenate([np.tile(block, l_pac // 4096), np.zeros(1, np.uint8)])
            _WORLDS[name] = World(None, [1 << 30, l_pac - (1 << 30)], pac=pac, l_pac=l_pac)
        else:
            raise KeyError(name)
    return _WORLDS[name]


class Rd:
    def __init__(self, tag, query, chains, before=None, after=None, route=None, tally=None, check=None, order_dep=False, frac=None):
        self.tag, self.query, self.chains = tag, [int(c) for c in query], [[tuple(int(v) for v in s) for s in c] for c in chains]
        self.before, self.after, self.route, self.tally, self.check, self.order_dep = before, after, route, dict(tally or {}), check, order_dep
        self.frac = frac if frac is not None else [(ci % 4) / 4.0 for ci in range(len(chains))]


class Part:
    """one call of the entry: a reference, options, reads; error = (code, word of the message) where the call must refuse"""

    def __init__(self, wd, reads, opt=None, error=None, ref_opt=None):
        self.wd, self.reads, self.opt, self.error, self.ref_opt = wd, reads, dict(opt or {}), error, dict(ref_opt or {})     # ref_opt: switches of the reference's tally

    def ropt(self):
        return rr.opt_from(**dict(self.opt, **self.ref_opt))

    def lib_opt(self, lib):
        o = lib.opt_init()
        for k, v in self.opt.items():
            o[k] = v
        if "a" in self.opt or "b" in self.opt:
            a, b = int(o["a"][0]), int(o["b"][0])
            o["mat"][0] = np.array([[(a if i == j else -b) if i < 4 and j < 4 else -1 for j in range(5)] for i in range(5)], dtype=np.int8).reshape(-1)
        return o

    def orc_opt(self, oracle):
        o = self.ropt()
        h = oracle.opt_scores(o["a"], o["b"], o["o_del"], o["e_del"], o["o_ins"], o["e_ins"])
        return oracle.opt_regions(h, o["w"], o["zdrop"], o["pen_clip5"], o["pen_clip3"], o["max_chain_gap"], float(o["mask_level_redun"]))

    def packed(self):
        """the reads' seeds are laid out in REVERSE of their chain order, so that a seed's index is not its place in the chain lists"""
        wd = self.wd
        seq = np.array([c for r in self.reads for c in r.query], dtype=np.uint8)
        off = np.zeros(len(self.reads) + 1, dtype=np.int64); off[1:] = np.cumsum([len(r.query) for r in self.reads])
        seed_off = np.zeros(len(self.reads) + 1, dtype=np.int64); seed_off[1:] = np.cumsum([sum(len(c) for c in r.chains) for r in self.reads])
        chain_off = np.zeros(len(self.reads) + 1, dtype=np.int64); chain_off[1:] = np.cumsum([len(r.chains) for r in self.reads])
        s4, ch3, cs = [], [], []
        for r in self.reads:
            flat = [s for c in r.chains for s in c]
            n = len(flat)
            s4 += [(s[0], s[1], s[2], 0) for s in reversed(flat)]
            k = 0
            for ci, c in enumerate(r.chains):
                ch3.append((wd.ref.rid_of(c[0][0]), len(c), int(np.float32(r.frac[ci]).view(np.uint32))))
                cs += [n - 1 - (k + j) for j in range(len(c))]
                k += len(c)
        s4 = np.array(s4, dtype=np.int64).reshape(-1, 4)
        ch3 = np.array(ch3, dtype=np.int64).reshape(-1, 3)
        seeds = np.zeros(len(s4), capi.SEED_DT)
        seeds["rbeg"], seeds["qbeg"], seeds["len"] = s4[:, 0], s4[:, 1], s4[:, 2]
        seeds["score"], seeds["next"] = 12345, 777      # (ignored by the entry)
        chains = np.zeros(len(ch3), capi.CHAIN_DT)
        chains["rid"], chains["n"] = ch3[:, 0], ch3[:, 1]
        chains["frac_rep"] = ch3[:, 2].astype(np.uint32).view(np.float32)
        chains["first_seed"] = np.concatenate([[0], np.cumsum(ch3[:, 1])[:-1]]) if len(ch3) else 0
        return dict(seq=seq, off=off, seed_off=seed_off, s4=s4, seeds=seeds, chain_off=chain_off, ch3=ch3, chains=chains, cs=np.array(cs, dtype=np.int32))


class Group:
    def __init__(self, name, aim, parts, order_dependent=False, near=False):
        self.name, self.aim, self.parts, self.order_dependent, self.near = name, aim, parts, order_dependent, near


def rows_of(regs):
    """region records as tuples over rr.FIELDS, frac_rep by its bits"""
    bits = regs["frac_rep"].view(np.uint32)
    return [tuple(int(bits[k]) if f == "frac_rep" else int(regs[f][k]) for f in rr.FIELDS) for k in range(len(regs))]


def rows_of_ref(lst):
    return [tuple(int(np.float32(x[f]).view(np.uint32)) if f == "frac_rep" else int(x[f]) for f in rr.FIELDS) for x in lst]


def run_oracle(oracle, part):
    p = part.packed()
    wd = part.wd
    ro, regs, nb = oracle.regions(wd.pac, wd.l_pac, wd.ctg_off, wd.ctg_len, p["seq"], p["off"], p["seed_off"], p["s4"], p["chain_off"], p["ch3"], p["cs"], opt=part.orc_opt(oracle))
    rows = rows_of(regs)
    return [rows[int(ro[r]):int(ro[r + 1])] for r in range(len(part.reads))], [int(x) for x in nb]


def run_library(lib, part):
    p = part.packed()
    wd = part.wd
    ro, regs, route = lib.dbg_regions(part.lib_opt(lib), wd.pac, wd.l_pac, wd.ctg_off, wd.ctg_len, p["seq"], p["off"], p["seed_off"], p["seeds"], p["chain_off"], p["chains"], p["cs"])
    rows = rows_of(regs)
    return [rows[int(ro[r]):int(ro[r + 1])] for r in range(len(part.reads))], [int(x) for x in route]


_REFS, COUNTS = {}, {}


def part_reference(part):
    out, t_all = [], rr.Tally()
    opt = part.ropt()
    for rd in part.reads:
        t = rr.Tally()
        lst, av = rr.regions(opt, part.wd.ref, rd.query, [(part.wd.ref.rid_of(c[0][0]), rd.frac[ci], c) for ci, c in enumerate(rd.chains)], t)
        out.append((None if lst is None else rows_of_ref(lst), len(av), t, lst, av))
        for k, v in t.c.items():
            t_all.add(k, v)
    return out, t_all


def group_reference(g):
    """every part of the group through the reference, once; what the group claims is asserted here, on the reference alone"""
    if g.name not in _REFS:
        res, cnt = [], dict(reads=0, chains=0, regions_before=0, regions_after=0, order_dependent=0, near=0, refused_calls=0, tally={})
        for part in g.parts:
            if part.error:
                res.append(None)
                cnt["refused_calls"] += 1
                continue
            refs, t = part_reference(part)
            res.append(refs)
            for rd, (rows, nb, tl, lst, av) in zip(part.reads, refs):
                ctx = (g.name, rd.tag)
                assert (rows is None) == bool(rd.order_dep), (ctx, "order-dependent" if rows is None else "decided", tl.c)
                if rd.before is not None:
                    assert nb == rd.before, (ctx, "regions before the dedup", nb, rd.before)
                if rd.after is not None and rows is not None:
                    assert len(rows) == rd.after, (ctx, "regions after the dedup", len(rows), rd.after, tl.c)
                for k, v in rd.tally.items():
                    assert (tl[k] >= 1) if v is True else (tl[k] == v), (ctx, k, tl.c)
                if rd.check is not None:
                    assert rd.check(lst, av), (ctx, "check", lst, av)
                cnt["reads"] += 1; cnt["chains"] += len(rd.chains); cnt["regions_before"] += nb
                cnt["regions_after"] += len(rows) if rows is not None else 0
                cnt["order_dependent"] += rows is None
            cnt["near"] += t.near()
            for k, v in t.c.items():
                cnt["tally"][k] = cnt["tally"].get(k, 0) + v
        if not g.order_dependent:
            assert cnt["order_dependent"] == 0, (g.name, "an order-dependent read outside the group built for them")
        else:
            assert cnt["order_dependent"] > 0, g.name
        if g.near:
            assert cnt["near"] > 0, (g.name, "no near site")
        COUNTS[g.name] = cnt
        _REFS[g.name] = res
    return _REFS[g.name]


_ORC = {}


def group_oracle(g, oracle):
    if g.name not in _ORC:
        _ORC[g.name] = [None if part.error else run_oracle(oracle, part) for part in g.parts]
    return _ORC[g.name]


def hold(rows, refs, part, who, gname):
    for r, (rd, got) in enumerate(zip(part.reads, rows)):
        want = refs[r][0]
        if want is None:
            continue
        if got != want:
            k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            raise AssertionError("%s: %s, read %s: %d regions against the reference's %d; first difference at %d: %s against %s (fields %s)"
                                 % (gname, who, rd.tag, len(got), len(want), k, got[k] if k < len(got) else None, want[k] if k < len(want) else None, rr.FIELDS))


def check_group_oracle(g, oracle):
    refs = group_reference(g)
    orc = group_oracle(g, oracle)
    for part, rf, oc in zip(g.parts, refs, orc):
        if part.error:
            continue
        rows, nb = oc
        assert nb == [x[1] for x in rf], (g.name, "regions before the dedup, oracle against reference")
        hold(rows, rf, part, "the oracle", g.name)


def check_group_library(g, lib, oracle, who):
    refs = group_reference(g)
    orc = group_oracle(g, oracle)
    routes = COUNTS[g.name].setdefault("routes_" + who.split()[1], {})
    for part, rf, oc in zip(g.parts, refs, orc):
        if part.error:
            with pytest.raises(capi.SsgError) as e:
                run_library(lib, part)
            assert str(part.error[0]) in str(e.value) and part.error[1] in str(e.value), (g.name, who, str(e.value))
            continue
        rows, route = run_library(lib, part)
        hold(rows, rf, part, who, g.name)
        assert rows == oc[0], (g.name, who, "against the oracle", [rd.tag for rd, a, b in zip(part.reads, rows, oc[0]) if a != b])
        for rd, rt in zip(part.reads, route):
            routes[str(rt)] = routes.get(str(rt), 0) + 1
            if rd.route is not None:
                assert rt == rd.route, (g.name, who, rd.tag, "route", rt, rd.route)


# ------------------------------------------------------------------------------------------------------------------------------
# the groups
# ------------------------------------------------------------------------------------------------------------------------------
def rnd(n, seed):
    return [int(x) for x in np.random.RandomState(seed).randint(0, 4, n)]


def far_chains(n, qb=5, ln=25, at=150000, step=1100):
    """n single-seed chains far from everything else (second contig of world `two'), nothing to do with the read: padding that sends a read to the wave kernel"""
    return [[(at + j * step, qb, ln)] for j in range(n)]


def patch_pair(wd, p, half, gap):
    """a read of 2 x half bases whose halves lie `gap' reference bases apart (a deletion the extension's band cannot cross), and the two seeds"""
    while wd.ref.base(p + half) == wd.ref.base(p + half + gap) or wd.ref.base(p + half - 1) == wd.ref.base(p + half + gap - 1):
        p += 1                                              # (a place where neither half runs on into the other by a chance match)
    q = wd.fw(p, half) + wd.fw(p + half + gap, half)
    return q, [(p + 2, 2, half - 4)], [(p + half + gap + 2, half + 2, half - 4)]


def patch_place(wd, p, half, gap):
    while wd.ref.base(p + half) == wd.ref.base(p + half + gap) or wd.ref.base(p + half - 1) == wd.ref.base(p + half + gap - 1):
        p += 1
    return p


def dup_pair(wd, p, u, d, v):
    """a read that carries d reference bases twice (u before, v behind): two regions that overlap by d on the reference and touch on the read, and the two seeds"""
    while wd.ref.base(p + u) == wd.ref.base(p + u + d) or wd.ref.base(p + u - 1) == wd.ref.base(p + u + d - 1):
        p += 1
    q = wd.fw(p, u + d) + wd.fw(p + u, d + v)
    return q, [(p + 2, 2, u + d - 4)], [(p + u + 2, u + d + 2, d + v - 4)]


def g_lane_limits():
    wd = world("two")
    q100 = rnd(100, 11)
    one = lambda j: [(j * 17000 + 1000, 10, 30)]
    reads = [Rd("six chains", q100, [one(j) for j in range(6)], before=6, route=0),
             Rd("seven chains", q100, [one(j) for j in range(7)], before=7, route=WAVE)]
    p = 5000
    q150 = wd.fw(p, 150)
    reads += [Rd("eight seeds", q150, [[(p + 15 * j, 15 * j, 20 + j) for j in range(8)]], before=1, after=1, route=0),
              Rd("nine seeds", q150, [[(p + 15 * j, 15 * j, 20 + j) for j in range(9)]], before=1, after=1, route=WAVE)]
    p = 30000
    q = wd.fw(p, 70) + wd.fw(p + 85, 80)                   # a deletion of 15 between two seeds of one chain, band 10
    reads.append(Rd("later seed extended", q, [[(60000, 5, 25)], [(p + 10, 10, 50), (p + 95, 80, 60)], [(90000, 100, 30)]], before=4, route=WAVE))
    reads.append(Rd("later seed contained", wd.fw(p, 150), [[(60000, 5, 25)], [(p + 10, 10, 50), (p + 80, 80, 60)], [(90000, 100, 30)]], before=3, route=0))
    parts = [Part(wd, reads, dict(w=10))]
    q, a, b = patch_pair(wd, 40000, 75, 3)
    parts.append(Part(wd, [Rd("patch candidate in the lane form", q, [a, b], before=2, after=1, route=WAVE | PATCH, tally=dict(patched=1)),
                           Rd("no candidate", q, [a, [(95000, 80, 40)]], before=2, after=2, route=0)], dict(w=2)))
    return Group("lane_limits", "6 / 7 chains, 8 / 9 seeds, a later seed extended, a patch candidate in the lane form", parts)


def g_seed_order():
    wd = world("two")
    p = 10000
    q = wd.fw(p, 150)
    reads = []
    for n in (1, 2, 3, 8, 9, 63, 64, 65, 200):
        # three seeds in five on the read's diagonal in its first 91 bases, two 4 off it in its last 55: no seed of one diagonal overlaps one of the other, so
        # nothing is revived into a twin of a region that is there already (twins tie in `re' and the read would be order-dependent)
        seeds = [(p + (i * 7) % 50, (i * 7) % 50, 19 + (i * 5) % 23) if i % 5 < 3 else (p + 95 + (i * 7) % 30 + 4, 95 + (i * 7) % 30, 19 + (i * 5) % 6) for i in range(n)]
        reads.append(Rd("%d seeds" % n, q, [seeds] + (far_chains(7) if n in (2, 8) else [])))
    reads.append(Rd("equal lengths: the higher index first", q, [[(p + 10, 10, 30), (p + 68, 60, 30)]], check=lambda lst, av: av[0]["rb"] - av[0]["qb"] == p + 8))
    reads.append(Rd("equal lengths, wave form", q, [[(p + 10, 10, 30), (p + 68, 60, 30)]] + far_chains(7), check=lambda lst, av: av[0]["rb"] - av[0]["qb"] == p + 8))
    reads.append(Rd("the best seed is the last of the chain", q, [[(p + 4, 10, 20), (p + 40, 40, 25), (p + 70, 70, 60)]], check=lambda lst, av: av[0]["seedlen0"] == 60))
    # sixty-five and more seeds of one length: the introsort's order among (score, index) keys is by index
    reads.append(Rd("70 seeds of one length", q, [[(p + i, i, 35) if i < 35 else (p + 40 + i + 7, 40 + i, 35) for i in range(70)]]))
    return Group("seed_order", "chains of 1 .. 200 seeds: ranks in registers (2 .. 64), the sort in global memory (65 and more), ties by index", [Part(wd, reads, dict(w=3))])


def g_contained():
    wd = world("two")
    p = 20000
    q150, q310 = wd.fw(p, 150), wd.fw(p, 310)
    pad = far_chains(7)
    reads = []
    for q, d, nb in ((q150, 15, 1), (q150, 16, 2), (q310, 31, 1), (q310, 32, 2)):
        for tag, extra in (("lane", []), ("wave", pad)):
            # (the longer seed lies one base off the diagonal: extended, it makes a region of its own score, not a twin of the first that ties with it)
            reads.append(Rd("seedlen0 + %d of %d, %s" % (d, len(q), tag), q, [[(p + 10, 10, 20)], [(p + 41, 40, 20 + d)]] + extra, before=nb + len(extra)))
    parts = [Part(wd, reads, dict(mask_level_redun=1000.0))]
    # band 5: offsets of 4 and 5 from the region's diagonal; near the region's start the flank (cal_max_gap) decides, at its end the band
    reads = []
    for d in (4, 5, -4, -5):
        for tag, extra in (("lane", []), ("wave", pad)):
            reads.append(Rd("offset %d, long flanks, %s" % (d, tag), q150, [[(p + 50, 50, 40)], [(p + 30 + d, 30, 30)]] + extra, before=(1 if abs(d) < 5 else 2) + len(extra)))
            reads.append(Rd("offset %d, short start flank, %s" % (d, tag), q150, [[(p + 50, 50, 40)], [(p + 8 + d, 8, 30)]] + extra, before=(1 if abs(d) < 5 else 2) + len(extra)))
            reads.append(Rd("offset %d, short end flank, %s" % (d, tag), q150, [[(p + 50, 50, 40)], [(p + 112 + d, 112, 30)]] + extra, before=(1 if abs(d) < 5 else 2) + len(extra)))
    # both flanks short: cal_max_gap of 7 bases is 2, below the band, and an offset of 2 is outside
    for d in (1, 2):
        reads.append(Rd("offset %d, both flanks short" % d, q150[:60], [[(p + 10, 10, 45)], [(p + 7 + d, 7, 44)]] + pad, before=(1 if d < 2 else 2) + len(pad)))
    # the walk: s (20 bases, 1 off the diagonal, contained) against t (30 bases, 8 off it, extended, live): an overlap of len >> 2 = 5 revives s, 4 does not
    # (s is off the diagonal so that, revived, it makes a region of a score of its own and no twin of the first)
    for ov, nb in ((5, 3), (4, 2)):
        for tag, extra in (("lane", []), ("wave", pad)):
            reads.append(Rd("walk, overlap %d, %s" % (ov, tag), q150, [[(p, 0, 50), (p + 100 - ov + 8, 100 - ov, 30), (p + 81, 80, 20)]] + extra, before=nb + len(extra)))
    # t is contained and marked; s would meet it off its diagonal, but a marked seed is skipped, so s is marked too
    for tag, extra in (("lane", []), ("wave", pad)):
        reads.append(Rd("walk, the marked seed is skipped, %s" % tag, q150, [[(p, 0, 50), (p + 63, 60, 30), (p + 80, 80, 20)]] + extra, before=1 + len(extra)))
    parts.append(Part(wd, reads, dict(w=5, mask_level_redun=1000.0)))
    return Group("contained", "the containment test: seedlen0 + 15 / 16 of 150 and 31 / 32 of 310, offsets at the band and one inside, short flanks, the walk", parts)


_TILE = 4096


def tiled_world(n_tiles, read, variants=None, seed=3):
    """n_tiles blocks of _TILE bases: random filler with `read' at offset 100; variants[j] = codes that replace tile j's copy (from offset 100)"""
    key = ("tiled", n_tiles, tuple(read), tuple(sorted((k, tuple(v)) for k, v in (variants or {}).items())), seed)
    if key not in _WORLDS:
        block = np.random.RandomState(seed).randint(0, 4, _TILE).astype(np.uint8)
        block[100:100 + len(read)] = read
        text = np.tile(block, n_tiles)
        for j, v in (variants or {}).items():
            text[j * _TILE + 100:j * _TILE + 100 + len(v)] = v
        _WORLDS[key] = World(text)
    return _WORLDS[key]


def g_scan_forms():
    read = rnd(40, 21)
    n = 2061
    wd = tiled_world(n, read)
    reg = lambda j: [(j * _TILE + 100 + 5, 5, 30)]              # region j: the whole read at tile j
    inside = lambda j: [(j * _TILE + 100 + 8 + 2, 8, 24)]       # a seed inside region j, 2 off its diagonal: cal_max_gap of 8 bases is 3
    chains = [reg(j) for j in range(2048)] + [inside(k) for k in (0, 447, 448, 449, 2047)] + [reg(2048)] + [inside(k) for k in (0, 448, 2048)] + [reg(j) for j in range(2049, n)]
    reads = [Rd("a seed inside region 0 .. 2048, all three forms of the scan", read, chains, before=n, after=n, route=WAVE | PATCH)]
    chains = [reg(j) for j in range(450)] + [inside(k) for k in (0, 447, 448, 449)]
    reads.append(Rd("450 regions: keys in LDS and in the slab", read, chains, before=450, after=450, route=WAVE))
    reads.append(Rd("not inside: 3 off the diagonal", read, [reg(j) for j in range(10)] + [[(3 * _TILE + 100 + 8 + 3, 8, 24)]], before=11, route=WAVE))
    parts = [Part(wd, reads, dict(mask_level_redun=1000.0))]
    # bins: (uint16_t)(rb >> 10) wraps every 2^26 bases -- a seed 2^26 bases behind a region has its bin and is not inside it
    ww = world("wide")
    p = 70000
    q = ww.fw(p, 100)
    pad = [[(30000 + 2000 * j, 5, 25)] for j in range(7)]
    reads = [Rd("rb 2^26 apart: equal bins", q, [[(p + 10, 10, 60)], [(p + (1 << 26) + 20, 20, 30)]] + pad, before=9, route=WAVE)]
    # a region that starts in the bin before the seed's
    p = 3 * 1024 - 10
    q = ww.fw(p, 100)
    reads.append(Rd("the region starts in the bin before", q, [[(p + 10, 10, 60)], [(p + 22, 20, 30)]] + pad, before=8, route=WAVE))
    reads.append(Rd("the region starts in the bin before, not inside", q, [[(p + 10, 10, 60)], [(p + 50, 20, 30)]] + pad, before=9, route=WAVE))
    parts.append(Part(ww, reads, dict(mask_level_redun=1000.0)))
    # a region of more than 1024 reference bases turns the bins off for the rest of the read (hq_ok = 0): -A 10 pays for a deletion of 715 bases
    wt = world("two")
    reads = []
    for span in (1024, 1025):
        p = 20000
        g_ = span - 310
        q = wt.fw(p, 155) + wt.fw(p + 155 + g_, 155)
        chains = [[(p + 50, 50, 60)]] + [[(60000 + 1300 * j, 5, 25)] for j in range(7)]
        chains += [[(p + 12, 10, 30)], [(60000 + 1300 * 3 + 2, 9, 19)], [(p + g_ + 200 + 2, 200, 30)], [(60000 + 1300 * 5 + 10 + 9, 10, 19)]]
        reads.append(Rd("a region of %d bases" % span, q, chains, before=8, route=WAVE, check=lambda lst, av, span=span: av[0]["re"] - av[0]["rb"] == span and av[0]["qe"] - av[0]["qb"] == 310))
    parts.append(Part(wt, reads, dict(a=10, w=1000, mask_level_redun=1000.0)))
    return Group("scan_forms", "the containment scan: bins in LDS, keys in LDS (448) and in the slab (2048), records above; bins that wrap; the bin before; no bins after a region of 1025 bases", parts)


def g_dedup_routes():
    read = rnd(150, 31)
    half, gap = 75, 3
    parts = []
    for n in (96, 97, 2048, 2049):
        # the last tile holds the two halves of the read 3 bases apart: a patch pair at the end of the list sorted by re
        last = np.concatenate([read[:half], rnd(gap, 5), read[half:]]).astype(np.uint8)
        wd = tiled_world(n + 1, read, {n - 1: last})
        reg = lambda j: [(j * _TILE + 100 + 2, 2, 146)]
        plain = [reg(j) for j in range(n)]
        # redundant pairs: a second chain one base off, at places of the sorted list that straddle its 64-entry blocks
        twins = [j for j in range(n - 40 if n > 200 else 64) if j % 64 in (0, 31, 63)][:40]
        redun = [reg(j) for j in range(n - len(twins))] + [[(j * _TILE + 100 + 2 + 1, 2, 146)] for j in twins]
        a, b = [((n - 1) * _TILE + 100 + 2, 2, half - 4)], [((n - 1) * _TILE + 100 + half + gap + 2, half + 2, half - 4)]
        late = [reg(j) for j in range(n - 2)] + [a, b]
        big = PATCH if n > 2048 else 0
        reads = [Rd("%d regions" % n, read, plain, before=n, after=n, route=WAVE | big, tally=dict(redundant=0, patch_aligned=0)),
                 Rd("%d regions, redundant pairs" % n, read, redun, before=n, after=n - len(twins), route=WAVE | big, tally=dict(redundant=len(twins), patch_aligned=0)),
                 Rd("%d regions, a patch at the end" % n, read, late, before=n, after=n - 1, route=WAVE | PATCH, tally=dict(patched=1))]
        parts.append(Part(wd, reads, dict(w=2)))
    return Group("dedup_routes", "96 / 97 / 2048 / 2049 regions into the dedup: LDS, slab, the general routine; redundant pairs across blocks; a late patch", parts)


def g_redundancy():
    wd = world("two")
    X = 50000
    reads = [Rd("19 of 20: not redundant in binary32", wd.fw(X, 20), [[(X, 0, 20)], [(X + 1, 0, 20)]], before=2, after=2, tally=dict(near_redun=True)),
             Rd("20 of 21: redundant", wd.fw(X, 21), [[(X, 0, 21)], [(X + 1, 0, 21)]], before=2, after=1),
             Rd("19 of 20, wave form", wd.fw(X, 20), [[(X, 0, 20)], [(X + 1, 0, 20)]] + far_chains(7, 2, 10), before=9, tally=dict(near_redun=True))]
    q = wd.fw(X, 100)
    strong, weak_before, weak_after = [(X + 2, 2, 96)], [(X + 1, 2, 96)], [(X + 5, 2, 96)]
    reads += [Rd("the later one is the better: the earlier goes", q, [weak_before, strong], before=2, after=1, check=lambda lst, av: lst[0]["score"] == 100),
              Rd("p.score < q.score: the later goes", q, [strong, weak_after], before=2, after=1, check=lambda lst, av: lst[0]["score"] == 100),
              Rd("three regions, the first exclusion changes the second", q, [[(X + 2, 2, 96)], [(X + 4, 2, 96)], [(X + 7, 2, 96)]], before=3),
              Rd("three regions, wave form", q, [[(X + 2, 2, 96)], [(X + 4, 2, 96)], [(X + 7, 2, 96)]] + far_chains(7), before=10)]
    parts = [Part(wd, reads)]
    # max_chain_gap: the pair of `patch_pair' lies 3 bases apart; with max_chain_gap 3 the later region is out of the scan's reach, with 4 it is patched
    q, a, b = patch_pair(wd, 40000, 75, 3)
    for mcg, after in ((3, 2), (4, 1)):
        parts.append(Part(wd, [Rd("rb at re + max_chain_gap%s" % ("" if mcg == 3 else " - 1"), q, [a, b], before=2, after=after, tally=dict(patched=2 - after)),
                               Rd("the same, wave form", q, [a, b] + far_chains(7), before=9, tally=dict(patched=2 - after))], dict(w=2, max_chain_gap=mcg)))
    # two contigs: the same pair across the boundary of the contigs is two regions of two contigs
    c1 = wd.ctg_off[1]
    q = wd.fw(c1 - 75, 75) + wd.fw(c1 + 3, 75)
    parts.append(Part(wd, [Rd("a pair across two contigs", q, [[(c1 - 73, 2, 71)], [(c1 + 5, 77, 71)]], before=2, after=2, tally=dict(patch_tried=0))], dict(w=2)))
    return Group("redundancy", "19 of 20 and 20 of 21, p.score < q.score, three regions, max_chain_gap and one less, two contigs", parts, near=True)


def g_patch():
    wd = world("two")
    L = wd.l_pac
    parts, reads = [], []
    q, a, b = patch_pair(wd, 40000, 125, 4)
    reads.append(Rd("gap, w = opt.w << 1", q, [a, b], before=2, after=1, route=WAVE | PATCH, tally=dict(patched=1),
                    check=lambda lst, av: lst[0]["n_comp"] == 3 and lst[0]["w"] == 8 and lst[0]["score"] == lst[0]["truesc"] == 250 - 10 and lst[0]["seedcov"] == 121))
    q, a, b = patch_pair(wd, 40000, 125, 5)
    reads.append(Rd("gap, w = (opt.w << 1) + 1", q, [a, b], before=2, after=2, tally=dict(patch_no_w=1)))
    q, a, b = patch_pair(wd, 40000, 28, 3)          # 3 / 59 = 0.0508
    reads.append(Rd("gap, r above 0.05f", q, [a, b], before=2, after=2, tally=dict(patch_no_r=1)))
    q, a, b = patch_pair(wd, 40000, 29, 3)          # 3 / 61 = 0.0492 < 0.05f
    reads.append(Rd("gap, r below 0.05f", q, [a, b], before=2, tally=dict(patch_aligned=1)))
    # not colinear: the later region on the reference is the earlier on the read
    q = wd.fw(41000, 75) + wd.fw(40900, 75)
    reads.append(Rd("not colinear", q, [[(41002, 2, 71)], [(40902, 77, 71)]], before=2, after=2, tally={"patch_no_not colinear": 1}))
    # the score ratio: one mismatch inside the later half lowers that region's score and the joined alignment alike (136 of an estimate of 148: patched);
    # 20 bases of another sequence around the junction are outside both regions (their ends are local) and inside the joined alignment: below 0.90f
    q, a, b = patch_pair(wd, 42000, 75, 3)
    pp = patch_place(wd, 42000, 75, 3)
    sa, sb = [(pp + 2, 2, 50)], [(pp + 75 + 3 + 100 - 75, 100, 45)]
    q1 = list(q); q1[90] = (q1[90] + 1) % 4
    reads.append(Rd("score ratio, one mismatch", q1, [sa, sb], before=2, after=1, tally=dict(patch_aligned=1, patched=1)))
    q2 = q[:65] + [3 - c for c in q[65:85]] + q[85:]
    reads.append(Rd("score ratio, 20 other bases around the junction", q2, [sa, sb], before=2, after=2, tally=dict(patch_aligned=1, patch_no_ratio=1)))
    # the reverse strand: the same pair read from the other side
    q, a, b = patch_pair(wd, 40000, 125, 4)
    pp = patch_place(wd, 40000, 125, 4)
    rq = rc(q)
    ra = [(2 * L - (pp + 125 + 4 + 125) + 2, 2, 121)]
    rb_ = [(2 * L - (pp + 125) + 2, 127, 121)]
    reads.append(Rd("a patch on the reverse strand", rq, [ra, rb_], before=2, after=1, route=WAVE | PATCH, tally=dict(patched=1), check=lambda lst, av: lst[0]["rb"] >= L))
    # a pair across l_pac: a region at the end of the forward strand, one at the start of the reverse strand
    q = wd.fw(L - 80, 75) + wd.fw(L + 5, 75)
    reads.append(Rd("a pair across l_pac", q, [[(L - 78, 2, 71)], [(L + 7, 77, 71)]], before=2, after=2, tally=dict(patch_no_strands=1)))
    # regions that overlap on the reference: w up to opt.w << 2, r below 0.05f x 2
    q, a, b = dup_pair(wd, 44000, 110, 8, 110)
    reads.append(Rd("overlap, w = opt.w << 2", q, [a, b], before=2, after=1, route=WAVE | PATCH, tally=dict(patched=1), check=lambda lst, av: lst[0]["w"] == 8 and lst[0]["n_comp"] == 3))
    q, a, b = dup_pair(wd, 44000, 110, 9, 110)
    reads.append(Rd("overlap, w = (opt.w << 2) + 1", q, [a, b], before=2, after=2, tally=dict(patch_no_w=1)))
    q, a, b = dup_pair(wd, 44000, 30, 8, 30)           # 8 / 68
    reads.append(Rd("overlap, r above 0.1f", q, [a, b], before=2, after=2, tally=dict(patch_no_r=1)))
    q, a, b = dup_pair(wd, 44000, 37, 8, 36)           # 8 / 81
    reads.append(Rd("overlap, r below 0.1f", q, [a, b], before=2, after=2, tally=dict(patch_aligned=1, patch_no_ratio=1)))
    parts.append(Part(wd, reads, dict(w=2)))
    # a merged window above 32768 bases: two regions of a few bases at the ends of a read of 310, 32768 reference bases apart; upstream aligns, the library refuses
    q = wd.fw(40000, 5) + rnd(300, 77) + wd.fw(40000 + 32768 + 5, 5)
    parts.append(Part(wd, [Rd("merged window above 32768", q, [[(40000, 0, 5)], [(40000 + 32768 + 5, 305, 5)]])], dict(w=16300, max_chain_gap=40000), error=(EOVERFLOW, "window")))
    return Group("patch", "mem_patch_reg: its early returns, w and r at their bounds, the score ratio, the merged fields, the reverse strand, across l_pac", parts)


def g_windows():
    wd = world("two")
    L = wd.l_pac
    c1 = wd.ctg_off[1]
    reads = []
    for tag, p in (("at 0", 0), ("at the contig's end", c1 - 150), ("at the contig's start", c1), ("at l_pac", L - 150), ("at l_pac on the reverse strand", L), ("at 2 l_pac", 2 * L - 150)):
        q = wd.fw(p, 150)
        for stag, s in (("seed at the start", (p, 0, 40)), ("seed inside", (p + 50, 50, 40)), ("seed at the end", (p + 110, 110, 40))):
            reads.append(Rd("%s, %s" % (tag, stag), q, [[s]], before=1, after=1))
        reads.append(Rd("%s, wave form" % tag, q, [[(p + 50, 50, 40), (p + 3, 5, 20), (p + 128, 125, 20)]] + [[(60000 + 900 * j, 5, 25)] for j in range(7)], route=WAVE))
    # a read that hangs over the cut: the window ends where the contig does, the extension runs out of reference
    q = wd.fw(c1 - 100, 100) + rnd(50, 41)
    reads.append(Rd("over the contig's end", q, [[(c1 - 90, 10, 60)]], before=1))
    q = rnd(50, 42) + wd.fw(c1, 100)
    reads.append(Rd("over the contig's start", q, [[(c1 + 10, 60, 60)]], before=1))
    parts = [Part(wd, reads)]
    # the window's span around the 1024 bases of the LDS window: at default scoring a window is at most 310 + 305 bases, so -A 3; the seed's place and the
    # cap of cal_max_gap (2 w) are searched for spans of 1023 .. 1026
    p = 20000
    q = wd.fw(p, 310)
    found = {}
    for w in range(200, 216):
        o = rr.opt_from(a=3, w=w)
        for qb in range(98, 104):
            lo, hi, _ = rr.window(o, wd.ref, 310, [(p + qb, qb, 30)])
            if 1023 <= hi - lo <= 1026 and hi - lo not in found:
                found[hi - lo] = (w, qb)
    assert sorted(found) == [1023, 1024, 1025, 1026], found
    for sp, (w, qb) in sorted(found.items()):
        parts.append(Part(wd, [Rd("window of %d bases" % sp, q, [[(p + qb, qb, 30)]], before=1),
                               Rd("window of %d bases, wave form, a later seed" % sp, q, [[(p + qb, qb, 30), (p + 140 + w, 140, 19), (p + 5, 5, 19)]] + [[(60000 + 1500 * j, 5, 25)] for j in range(7)],
                                  route=WAVE)], dict(a=3, w=w)))
    return Group("windows", "the window: cut at 0, at contig ends, at l_pac from either side, at 2 l_pac; spans around the LDS window's 1024 bases", parts)


def g_extension_classes():
    wd = world("two")
    parts = []
    for si, sc in enumerate((dict(), dict(o_del=7, o_ins=9, e_del=2, e_ins=1), dict(a=2, b=5))):
        reads = []
        p = 70000 + 1000 * si
        q310 = wd.fw(p, 310)
        mm = list(q310)
        for k in (3, 30, 77, 200, 290):
            mm[k] = (mm[k] + 1) % 4
        for side in (0, 1, 39, 40, 41, 72, 73, 80, 81, 248, 249, 291):
            reads.append(Rd("left side %d" % side, q310, [[(p + side, side, 19)]], before=1))
            reads.append(Rd("right side %d" % side, mm, [[(p + 310 - 19 - side, 310 - 19 - side, 19)]], before=1))
        q150 = wd.fw(p, 150)
        for side in (0, 1, 39, 40, 41, 72, 73, 80, 81):
            reads.append(Rd("150 bases, left side %d" % side, q150, [[(p + side, side, 19)]], before=1))
        # an insertion and a deletion of 8 / 12 bases beside the seed: the band decides whether the extension crosses (retry taken or not)
        for g_ in (6, 7, 8, 11, 12, 15, 16):
            qd = wd.fw(p, 60) + wd.fw(p + 60 + g_, 90)
            # a gap of g in a band of 10: crossed in the first try up to 10, and max_off = g reaches (10 >> 1) + (10 >> 2) = 7 at 7: retry at 7 and 8, none at 6;
            # beyond the band the first try stays on its diagonal (max_off 0) and there is no second
            rt = dict(retry=1 if g_ in (7, 8) else 0)
            reads.append(Rd("deletion of %d right of the seed" % g_, qd, [[(p + 20, 20, 30)]], before=1, tally=rt))
            qi = wd.fw(p, 60) + rnd(g_, 50 + g_) + wd.fw(p + 60, 90)
            reads.append(Rd("insertion of %d right of the seed" % g_, qi, [[(p + 20, 20, 30)]], before=1, tally=rt))
            ql = wd.fw(p, 90) + wd.fw(p + 90 + g_, 60)
            reads.append(Rd("deletion of %d left of the seed" % g_, ql, [[(p + 110 + g_, 110, 30)]], before=1, tally=rt))
            # a later seed of a chain, extended by the wave kernel's own DP: the same indel beside it
            reads.append(Rd("deletion of %d right of a later seed" % g_, qd, [[(p + 90 + g_, 90, 40), (p + 20, 20, 30)]] + far_chains(7), route=WAVE))
        # gscore at score - pen_clip and one above: a mismatch k bases from the read's end leaves gscore = score - b + (k - 1) a, on the edge (local) where
        # (k - 1) a - b = -pen_clip: k = 1 under -A 2 -B 5, no k under -A 1 -B 4 with a clipping penalty of 5 (the part below lowers it to 3: k = 2)
        for k in range(1, 9):
            eg = dict(edge_gscore=1 if (k - 1) * sc.get("a", 1) - sc.get("b", 4) == -5 else 0)
            qe = list(q150)
            qe[150 - k] = (qe[150 - k] + 1) % 4
            reads.append(Rd("mismatch %d from the 3' end" % k, qe, [[(p + 50, 50, 40)]], before=1, tally=eg))
            qs = list(q150)
            qs[k - 1] = (qs[k - 1] + 1) % 4
            reads.append(Rd("mismatch %d from the 5' end" % k, qs, [[(p + 50, 50, 40)]], before=1, tally=eg))
            # the same through the wave kernel, and with a second seed of the chain that it has to extend itself (5 off the diagonal, band 10, short flank)
            reads.append(Rd("mismatch %d from the 3' end, wave form" % k, qe, [[(p + 50, 50, 40), (p + 3 + 5, 3, 30)]] + far_chains(7), route=WAVE))
            reads.append(Rd("mismatch %d from the 5' end, wave form" % k, qs, [[(p + 50, 50, 40), (p + 117 + 5, 117, 30)]] + far_chains(7), route=WAVE))
        # z-drop (100): a tail of another sequence ends the right side early once the row maximum has fallen 100 below the best -- never within 20 bases (at most
        # 5 a base), always within 100 (2.75 a base and more on average)
        for at in (20, 60, 100):
            qz = wd.fw(p, 310 - at) + rnd(at, 60 + at)
            reads.append(Rd("random tail of %d" % at, qz, [[(p + 10, 10, 25)]], before=1, tally={} if at == 60 else dict(zdrop_ended=1 if at == 100 else 0)))
        parts.append(Part(wd, reads, dict(sc, w=10), ref_opt=dict(count_zdrop=True)))
    # -A 1 -B 4 with a clipping penalty of 3: the edge is at k = 2 (gscore = score - 3: local), k = 3 is one above (to the end)
    p = 74000
    q150 = wd.fw(p, 150)
    reads = []
    for k in range(1, 5):
        qe = list(q150); qe[150 - k] = (qe[150 - k] + 1) % 4
        qs = list(q150); qs[k - 1] = (qs[k - 1] + 1) % 4
        eg = dict(edge_gscore=1 if k == 2 else 0, to_end=1 if k <= 2 else 2)
        reads.append(Rd("clipping penalty 3, mismatch %d from the 3' end" % k, qe, [[(p + 50, 50, 40)]], before=1, tally=eg))
        reads.append(Rd("clipping penalty 3, mismatch %d from the 5' end" % k, qs, [[(p + 50, 50, 40)]], before=1, tally=eg))
        reads.append(Rd("clipping penalty 3, mismatch %d from the 3' end, wave form" % k, qe, [[(p + 50, 50, 40), (p + 3 + 5, 3, 30)]] + far_chains(7), route=WAVE))
    parts.append(Part(wd, reads, dict(w=10, pen_clip5=3, pen_clip3=3)))
    return Group("extension_classes", "side lengths at the column classes, three scoring sets, the band retry, gscore against score - pen_clip, z-drop", parts)


def big_band_reads(wd):
    """one read three ways: a contained seed (2 off the diagonal of region 0) met by the wave form among the first 448 regions, beyond them, and by the lane form"""
    p = 20000
    q = wd.fw(p, 150)
    base, inside = [(p + 10, 10, 60)], [(p + 82, 80, 30)]
    many = [[(60000 + 300 * j, 5, 25)] for j in range(460)]
    return [Rd("wave form, first 448 regions", q, [base] + many[:7] + [inside], before=8, route=WAVE),
            Rd("wave form, beyond region 448", q, many[:450] + [base] + [inside], before=451, route=WAVE),
            Rd("lane form", q, [base, inside], before=1, route=0)]


def g_big_band():
    wd = world("two")
    parts = [Part(wd, big_band_reads(wd), dict(w=w, mask_level_redun=1000.0)) for w in (100, 32767, 32768, 65535)]
    parts += [Part(wd, big_band_reads(wd), dict(w=w, mask_level_redun=1000.0), error=(EINVAL, "65535")) for w in (65536, 100000)]
    return Group("big_band", "-w up to 65535 equals the reference; above, the call refuses: a region's band travels in 16 bits through the wave kernel's keys", parts)


def g_high_positions():
    wd = world("high")
    reads = []
    pad = [[(150000 + 1100 * j, 5, 25)] for j in range(7)]
    for tag, p in (("forward strand above 2^31", (1 << 31) + 500), ("across 2^31", (1 << 31) - 75), ("reverse strand", wd.l_pac + 3000),
                   ("across 2^32", (1 << 32) - 75), ("reverse strand above 2^32", (1 << 32) + 300)):
        q = wd.fw(p, 150)
        reads.append(Rd(tag, q, [[(p + 50, 50, 40)]], before=1, after=1, route=0, check=lambda lst, av, p=p: (lst[0]["rb"], lst[0]["re"]) == (p, p + 150)))
        reads.append(Rd(tag + ", a later seed, wave form", q, [[(p + 50, 50, 40), (p + 5 + 4, 5, 30)]] + pad, route=WAVE))
        reads.append(Rd(tag + ", the dedup", q, [[(p + 2, 2, 146)], [(p + 5, 2, 146)], [(p + 1, 2, 146)]], before=3, after=1, tally=dict(redundant=2)))
        reads.append(Rd(tag + ", the dedup, wave form", q, [[(p + 2, 2, 146)], [(p + 5, 2, 146)], [(p + 1, 2, 146)]] + pad, before=10, tally=dict(redundant=2), route=WAVE))
        q, a, b = patch_pair(wd, p, 75, 3)
        reads.append(Rd(tag + ", a patch", q, [a, b], before=2, after=1, route=WAVE | PATCH, tally=dict(patched=1)))
        reads.append(Rd(tag + ", a patch among more regions", q, pad + [a, b], before=9, after=8, route=WAVE | PATCH, tally=dict(patched=1)))
    return Group("high_positions", "l_pac above 2^31: chains, the dedup and a patch above 2^31 and 2^32 in doubled coordinates, on both strands", [Part(wd, reads, dict(w=2))])


def g_order_dependent():
    wd = world("two")
    X = 50000
    q = wd.fw(X, 100)
    # two regions of one `re', one score and one `rb' that differ in seedlen0 and seedcov: which survives is the sort's choice
    # (the second chain's seed is 11 bases longer than the first region's seedlen0, more than a tenth of the read: not inside, extended to the same region)
    reads = [Rd("equal re and equal (score, rb, qb)", q, [[(X + 10, 10, 20)], [(X + 40, 40, 31)]], before=2, order_dep=True),
             Rd("the same, wave form", q, [[(X + 10, 10, 20)], [(X + 40, 40, 31)]] + far_chains(7), before=9, order_dep=True),
             Rd("equal re, different scores: decided", q, [[(X + 10, 10, 20)], [(X + 41, 40, 31)]], before=2, after=1)]
    return Group("order_dependent", "ties in re and in (score, rb, qb) that change the list: the reference reports them, the builds agree with one another", [Part(wd, reads)],
                 order_dependent=True)


GROUPS = dict((f.__name__[2:], f) for f in (g_lane_limits, g_seed_order, g_contained, g_scan_forms, g_dedup_routes, g_redundancy, g_patch, g_windows, g_extension_classes,
                                             g_big_band, g_high_positions, g_order_dependent))
GROUP_NAMES = list(GROUPS)
_GROUPS = {}


def group(name):
    if name not in _GROUPS:
        _GROUPS[name] = GROUPS[name]()
    return _GROUPS[name]


# ------------------------------------------------------------------------------------------------------------------------------
# leg 1: the reference against itself
# ------------------------------------------------------------------------------------------------------------------------------
def test_cal_max_gap_and_the_band_of_the_patch():
    o = rr.opt_from()
    assert [rr.cal_max_gap(o, n) for n in (0, 5, 6, 7, 100, 205, 206, 300)] == [1, 1, 1, 2, 95, 200, 200, 200]
    o = rr.opt_from(o_del=7, e_del=2, o_ins=9, e_ins=1, w=3)
    assert [rr.cal_max_gap(o, n) for n in (0, 9, 10, 11, 12, 40)] == [1, 2, 2, 3, 4, 6]       # (n - 7) / 2 + 1 against n - 9 + 1, capped at 6
    for n in range(0, 320):        # the exact quotient is the double's: no length is near
        for oo in (rr.opt_from(), o, rr.opt_from(a=2, b=5)):
            for op, ex in ((oo["o_del"], oo["e_del"]), (oo["o_ins"], oo["e_ins"])):
                assert int(float(n * oo["a"] - op) / ex + 1.) == rr.trunc(F(n * oo["a"] - op, ex) + 1)
    assert rr.gen_band(rr.opt_from(), 150, 153, 8) == 8 and rr.gen_band(rr.opt_from(), 150, 153, 2) == 6 and rr.gen_band(rr.opt_from(), 10, 10, 400) == 3


def test_where_the_near_sites_are():
    m = np.float32(0.95)
    assert np.float32(m * np.float32(20)) == np.float32(19.0) and float(m) * 20 < 19            # rounded: 19.0; exact: 18.99999976
    assert not np.float32(19) > m * np.float32(20) and F(19) > rr.f32(F(95, 100)) * 20            # not redundant in binary32, redundant exactly
    assert np.float32(20) > m * np.float32(21) and F(20) > rr.f32(F(95, 100)) * 21
    t = rr.Tally()
    p, q = dict(rb=1, re=21, qb=0, qe=20, score=20), dict(rb=0, re=20, qb=0, qe=20, score=20)
    assert not rr.redundant(rr.opt_from(), p, q, t) and t["near_redun"] == 1
    # every shorter side up to 310 with the overlap next to 0.95 of it: the sites where binary32 and the exact product part
    near = [n for n in range(1, 311) for o in (int(0.95 * n), int(0.95 * n) + 1) if (np.float32(o) > m * np.float32(n)) != (F(o) > rr.f32(F(95, 100)) * n)]
    assert near == [20, 40, 60, 80, 100, 120, 140, 160, 180, 200, 220, 240, 260, 280, 300], near
    # the two binary64 products: no read length puts an integer on the other side of .1 * l or .95 * l than the exact constant does
    for n in range(1, 311):
        for k in (int(0.1 * n), int(0.1 * n) + 1):
            assert (k > 0.1 * n) == (k > rr.D_01 * n)
        for k in (int(0.95 * n), int(0.95 * n) + 1):
            assert (k < n * 0.95) == (k < rr.D_095 * n)
    assert float(rr.F_005) == float(np.float32(0.05)) and float(rr.F_090) == float(np.float32(0.90)) and float(2 * rr.F_005) == float(np.float32(0.05) * np.float32(2))


def test_the_walks_length_test_is_dead_while_a_seeds_score_is_its_length():
    """t.len < s.len * .95 is asked of seeds of HIGHER rank only, and the rank is (score, index) with score = len (bwa 0.7.12): t.len >= s.len always, so the
    test never holds, whatever the constant: a t of 19 bases is never asked about an s of 20 (19 < 19.0 would be false upstream as well)."""
    t = rr.Tally()
    for sl in range(1, 311):
        for tl in range(sl, min(sl + 3, 311)):
            assert not rr._lt_prod64(tl, rr.D_095, sl, t, "near_walk")
    assert t.near() == 0


def test_seedcov_against_position_sets():
    rs = np.random.RandomState(7)
    for _ in range(300):
        seeds = [(int(rs.randint(1000, 1100)), int(rs.randint(0, 100)), int(rs.randint(1, 50))) for _ in range(int(rs.randint(1, 12)))]
        a = dict(rb=int(rs.randint(990, 1060)), qb=int(rs.randint(0, 50)))
        a["re"], a["qe"] = a["rb"] + int(rs.randint(1, 120)), a["qb"] + int(rs.randint(1, 120))
        want = 0
        for rb, qb, ln in seeds:      # a seed counts when every one of its positions, on both axes, is a position of the region
            if set(range(rb, rb + ln)) <= set(range(a["rb"], a["re"])) and set(range(qb, qb + ln)) <= set(range(a["qb"], a["qe"])):
                want += ln
        assert rr.seedcov(seeds, a) == want
    assert rr.seedcov([(10, 0, 5), (10, 0, 5)], dict(rb=10, re=15, qb=0, qe=5)) == 10           # two equal seeds are two seeds


def test_window_against_a_per_base_union():
    wd = world("two")
    L, c1 = wd.l_pac, wd.ctg_off[1]
    rs = np.random.RandomState(8)
    for o in (rr.opt_from(), rr.opt_from(w=3), rr.opt_from(a=2, b=5, o_del=7, e_del=2)):
        for _ in range(200):
            lq = int(rs.randint(20, 311))
            anchor = int(rs.choice([0, 100, c1 - 200, c1 - 10, c1, c1 + 50, L - 200, L - 5, L, L + 100, 2 * L - 320]))
            seeds = []
            for _ in range(int(rs.randint(1, 5))):
                ln = int(rs.randint(1, lq + 1)); qb = int(rs.randint(0, lq - ln + 1)); rb = min(max(anchor + int(rs.randint(0, 300)), 0), 2 * L - ln)
                seeds.append((rb, qb, ln))
            lo, hi, rid = rr.window(o, wd.ref, lq, seeds)
            cover = set()
            for rb, qb, ln in seeds:
                cover |= set(range(rb - qb - rr.cal_max_gap(o, qb), rb + ln + (lq - qb - ln) + rr.cal_max_gap(o, lq - qb - ln)))
            f = seeds[0][0]
            same = lambda x: 0 <= x < 2 * L and (x < L) == (f < L) and wd.ref.rid_of(x) == wd.ref.rid_of(f)
            keep = set(x for x in range(min(cover), max(cover) + 1) if same(x))     # the hull of the union, then the bases of the first seed's strand and contig
            assert rid == wd.ref.rid_of(f)
            assert (lo, hi) == (min(keep), max(keep) + 1) and keep == set(range(lo, hi)), (seeds, lo, hi)


def test_hand_worked_chains():
    text = np.array(rnd(400, 9), dtype=np.uint8)
    wd = World(text)
    o = rr.opt_from()
    q = wd.fw(100, 50)
    # a perfect read, one seed inside: 10 bases to the left at 1 each, 20 to the right; both sides reach the end (gscore = score > score - 5)
    lst, av = rr.regions(o, wd.ref, q, [(0, 0.5, [(110, 10, 20)])])
    assert len(av) == 1 and lst == av
    a = av[0]
    assert (a["rb"], a["re"], a["qb"], a["qe"], a["score"], a["truesc"], a["w"], a["seedcov"], a["seedlen0"], a["n_comp"], a["frac_rep"]) == (100, 150, 0, 50, 50, 50, 100, 20, 20, 0, 0.5)
    # a second seed on the diagonal is inside the region: nothing more; one 7 off it, with 30 bases before it (cal_max_gap 25, band 100): outside
    lst, av = rr.regions(o, wd.ref, q, [(0, 0.0, [(110, 10, 20), (135, 35, 10)])])
    assert len(av) == 1 and av[0]["seedcov"] == 30
    # a seed that is the whole read: no extension, score = len x a
    lst, av = rr.regions(o, wd.ref, q, [(0, 0.0, [(100, 0, 50)])])
    assert (av[0]["score"], av[0]["truesc"], av[0]["rb"], av[0]["re"], av[0]["w"]) == (50, 50, 100, 150, 100)
    # a mismatch 4 bases from the 3' end: to the end scores 49 - 4 = 45, local 46, and 45 > 46 - 5: to the end; the local score stays `score'
    q2 = list(q); q2[46] = (q2[46] + 1) % 4
    lst, av = rr.regions(o, wd.ref, q2, [(0, 0.0, [(110, 10, 20)])])
    assert (av[0]["qe"], av[0]["re"], av[0]["score"], av[0]["truesc"]) == (50, 150, 46, 45)
    # ... with a clipping penalty of 2, 45 > 44: still to the end; of 1, 45 <= 45: local (the `<=' of local against to-end)
    lst, av = rr.regions(rr.opt_from(pen_clip3=2), wd.ref, q2, [(0, 0.0, [(110, 10, 20)])])
    assert (av[0]["qe"], av[0]["re"], av[0]["score"], av[0]["truesc"]) == (50, 150, 46, 45)
    t = rr.Tally()
    lst, av = rr.regions(rr.opt_from(pen_clip3=1), wd.ref, q2, [(0, 0.0, [(110, 10, 20)])], t)
    assert (av[0]["qe"], av[0]["re"], av[0]["score"], av[0]["truesc"]) == (46, 146, 46, 46) and t["edge_gscore"] == 1
    assert rr.to_end(45, 50, 5) is False and rr.to_end(46, 50, 5) is True and rr.to_end(0, -3, 5) is False
    # a second chain with the same seed: inside the first chain's region, no region of its own (the list is the read's, not the chain's)
    lst, av = rr.regions(o, wd.ref, q, [(0, 0.0, [(110, 10, 20)]), (0, 0.0, [(110, 10, 20)])])
    assert len(av) == 1
    # one base off the diagonal with 2 bases of flank (cal_max_gap 1): not inside; its region is redundant with the first, the dedup keeps the better, n_comp 1
    lst, av = rr.regions(o, wd.ref, q, [(0, 0.0, [(102, 2, 46)]), (0, 0.0, [(103, 2, 46)])])
    assert len(av) == 2 and len(lst) == 1 and lst[0]["n_comp"] == 1 and lst[0]["score"] == 50


def test_tie_groups_under_every_order():
    text = np.array(rnd(400, 9), dtype=np.uint8)
    wd = World(text)
    o = rr.opt_from()
    base = dict.fromkeys(rr.FIELDS, 0)
    mk = lambda **kw: dict(base, **kw)
    q = wd.fw(100, 50)
    # equal `re', far apart on the read: every order leaves the same list
    a, b = mk(rb=100, re=150, qb=0, qe=20, score=20, w=100), mk(rb=130, re=150, qb=30, qe=50, score=19, w=100)
    t = rr.Tally()
    out = rr.sort_dedup_patch(o, wd.ref, q, [a, b], t)
    assert [x["score"] for x in out] == [20, 19] and t["tie_reads_decided"] == 1
    assert rr.sort_dedup_patch(o, wd.ref, q, [b, a]) == out
    # equal `re', equal score, redundant: which one goes is the order's choice, and they differ in seedlen0
    a, b = mk(rb=100, re=150, qb=0, qe=50, score=50, w=100, seedlen0=20), mk(rb=100, re=150, qb=0, qe=50, score=50, w=100, seedlen0=30)
    t = rr.Tally()
    assert rr.sort_dedup_patch(o, wd.ref, q, [a, b], t) is None and t["order_dependent"] == 1
    # ... and decided when they are equal in every field
    assert rr.sort_dedup_patch(o, wd.ref, q, [a, dict(a)]) == [dict(a, n_comp=1)]
    # equal (score, rb, qb) in the second sort, different `re': the identical-hit pass drops the later of the two, whichever that is
    a, b = mk(rb=100, re=130, qb=0, qe=30, score=30, w=100, rid=0), mk(rb=100, re=150, qb=0, qe=50, score=30, w=100, rid=0)
    assert rr.sort_dedup_patch(rr.opt_from(mask_level_redun=1000.0), wd.ref, q, [a, b]) is None
    # a group of five is beyond the cap
    five = [mk(rb=100 + k, re=150, qb=k, qe=k + 10, score=10 + k, w=100) for k in range(5)]
    t = rr.Tally()
    assert rr.sort_dedup_patch(o, wd.ref, q, five, t) is None and t["ties_beyond_caps"] == 1
    # n <= 1: returned untouched, n_comp stays 0
    assert rr.sort_dedup_patch(o, wd.ref, q, [a]) == [a]


# ------------------------------------------------------------------------------------------------------------------------------
# leg 2: constructed groups
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GROUP_NAMES)
def test_oracle_group_against_reference(name, oracle):
    check_group_oracle(group(name), oracle)


@pytest.mark.parametrize("name", GROUP_NAMES)
def test_emu_group_against_reference(name, emu_lib, oracle):
    check_group_library(group(name), emu_lib, oracle, "the emulation build")


@pytest.mark.gpu
@pytest.mark.parametrize("name", GROUP_NAMES)
def test_gpu_group_against_reference(name, gpu_lib, oracle):
    check_group_library(group(name), gpu_lib, oracle, "the HIP build")


def test_validation_of_the_entry(emu_lib):
    wd = world("two")
    part = Part(wd, [Rd("v", wd.fw(1000, 100), [[(1010, 10, 30), (1050, 50, 20)], [(130000, 5, 25)]])])
    p = part.packed()

    def call(**kw):
        a = dict(p, opt=emu_lib.opt_init(), l_pac=wd.l_pac, ctg_off=wd.ctg_off, ctg_len=wd.ctg_len)
        a.update(kw)
        return emu_lib.dbg_regions(a["opt"], wd.pac, a["l_pac"], a["ctg_off"], a["ctg_len"], a["seq"], a["off"], a["seed_off"], a["seeds"], a["chain_off"], a["chains"], a["cs"])
    call()

    def changed(a, f, v, k=0):
        b = a.copy()
        if f is None:
            b[k] = v
        else:
            b[f][k] = v
        return b

    def opt_with(**kw):
        o = emu_lib.opt_init()
        for k, v in kw.items():
            o[k] = v
        return o
    bad = [dict(off=np.array([0, 0], np.int64)), dict(off=np.array([1, 100], np.int64)), dict(seed_off=np.array([3, 0], np.int64)), dict(chain_off=np.array([1, 2], np.int64)),
           dict(seq=changed(p["seq"], None, 5)), dict(seeds=changed(p["seeds"], "qbeg", -1)), dict(seeds=changed(p["seeds"], "len", 0)), dict(seeds=changed(p["seeds"], "qbeg", 90)),
           dict(seeds=changed(p["seeds"], "rbeg", -1)), dict(seeds=changed(p["seeds"], "rbeg", 2 * wd.l_pac - 19)), dict(chains=changed(p["chains"], "n", 0)),
           dict(chains=changed(p["chains"], "rid", 1)), dict(chains=changed(p["chains"], "first_seed", 1)), dict(cs=changed(p["cs"], None, 3)), dict(cs=changed(p["cs"], None, 1)),
           dict(l_pac=0), dict(ctg_len=[120000, 79999]), dict(opt=opt_with(w=65536)), dict(opt=opt_with(w=-1)), dict(opt=opt_with(a=32)), dict(opt=opt_with(b=33))]
    for k, kw in enumerate(bad):
        with pytest.raises(capi.SsgError, match="-22"):
            call(**kw)
            raise AssertionError("case %d was accepted" % k)
    # every seed of a chain inside the contig and strand of the chain's first seed: across the contigs' boundary, on the other contig, across l_pac, on the other strand
    c1, L = wd.ctg_off[1], wd.l_pac
    for rb in (c1 - 10, c1 + 500, L - 10, 2 * L - 1100):
        with pytest.raises(capi.SsgError, match="-22.*contig and strand"):
            call(seeds=changed(p["seeds"], "rbeg", rb, k=1))          # (seeds[1] is the second seed of the first chain: the layout is reversed)
    big = np.concatenate([wd.fw(1000, 100), [0] * 211]).astype(np.uint8)
    with pytest.raises(capi.SsgError, match="-22"):
        call(seq=big, off=np.array([0, 311], np.int64))


def test_window_beyond_the_global_slab_is_refused(emu_lib):
    """a chain whose window exceeds 32768 bases returns SSG_EOVERFLOW and never a list: the seeds of a chain may lie anywhere, the window is their hull"""
    wd = world("two")
    part = Part(wd, [Rd("ok", wd.fw(1000, 100), [[(1010, 10, 30)]]), Rd("wide", wd.fw(1000, 100), [[(1010, 10, 30), (1010 + 32768, 50, 20)]])], error=(EOVERFLOW, "window"))
    with pytest.raises(capi.SsgError) as e:
        run_library(emu_lib, part)
    assert "-75" in str(e.value) and "window" in str(e.value)


@pytest.mark.gpu
def test_gpu_window_beyond_the_global_slab_is_refused(gpu_lib):
    wd = world("two")
    part = Part(wd, [Rd("ok", wd.fw(1000, 100), [[(1010, 10, 30)]]), Rd("wide", wd.fw(1000, 100), [[(1010, 10, 30), (1010 + 32768, 50, 20)]])], error=(EOVERFLOW, "window"))
    with pytest.raises(capi.SsgError) as e:
        run_library(gpu_lib, part)
    assert "-75" in str(e.value) and "window" in str(e.value)


# ------------------------------------------------------------------------------------------------------------------------------
# leg 3: the chains of simulated reads, and the composition of the test entries
# ------------------------------------------------------------------------------------------------------------------------------
_REAL = {}
REAL_SETS = dict(slice=(150, 41), repeat_mid=(30, 42))     # pairs, simulation seed: chosen on the CPU so that at most 5 % of a set's reads are order-dependent


def read_index_files(prefix):
    ann = open(prefix + ".ann").read().split("\n")
    l_pac, n_seq = int(ann[0].split()[0]), int(ann[0].split()[1])
    pac = np.fromfile(prefix + ".pac", dtype=np.uint8)[:l_pac // 4 + 1]
    if len(pac) < l_pac // 4 + 1:
        pac = np.concatenate([pac, np.zeros(l_pac // 4 + 1 - len(pac), np.uint8)])
    ctg = [(int(ann[2 + 2 * i].split()[0]), int(ann[2 + 2 * i].split()[1])) for i in range(n_seq)]
    return World(None, [c[1] for c in ctg], pac=pac, l_pac=l_pac)


def library_chains(lib, prefix, seq, off):
    """seeds and chains of the reads as the library's own stages leave them: ssg_seeds_batch -> ssg_dbg_chain"""
    idx = lib.index_load(prefix)
    opt = lib.opt_init()
    lib.l.ssg_index_n_ctg.argtypes = [type(idx)]
    l_pac, n_ctg = int(lib.l.ssg_index_l_pac(idx)), int(lib.l.ssg_index_n_ctg(idx))
    so, sd, rd = lib.seeds_batch(idx, opt, seq, off)
    cap = 4096
    li, ln = lib.smem_batch(idx, opt, seq, off, cap=cap)
    intv_off = np.zeros(len(ln) + 1, dtype=np.int64); intv_off[1:] = np.cumsum(ln)
    intv = np.concatenate([li[r, :ln[r]] for r in range(len(ln))]) if len(ln) else np.zeros(0, capi.INTV_DT)
    co, ch, cs, _ = lib.dbg_chain(opt, l_pac, n_ctg, np.diff(off).astype(np.int32), so, sd, rd, intv_off, intv)
    ro, regs, st = lib.align1_batch(idx, opt, seq, off)
    lib.index_destroy(idx)
    return dict(seed_off=so, seeds=sd, chain_off=co, chains=ch, cs=cs, reg_off=ro, regs=regs)


def check_realistic(lib, oracle, prefix, tag, who):
    n_pairs, seed = REAL_SETS[tag]
    wd = read_index_files(prefix)
    _, seqs, seq, off = common.sim_reads(n_pairs, seed, 150, fasta=prefix)
    c = library_chains(lib, prefix, seq, off)
    # composition: the test entries in a row are the pipeline's stage 1, field for field
    ro, regs, route = lib.dbg_regions(lib.opt_init(), wd.pac, wd.l_pac, wd.ctg_off, wd.ctg_len, seq, off, c["seed_off"], c["seeds"], c["chain_off"], c["chains"], c["cs"])
    assert np.array_equal(ro, c["reg_off"]), (who, tag)
    assert rows_of(regs) == rows_of(c["regs"]), (who, tag)
    # the same chains through the reference (once) and the oracle
    if tag not in _REAL:
        reads = []
        for r in range(len(seqs)):
            chains = []
            for k in range(int(c["chain_off"][r]), int(c["chain_off"][r + 1])):
                x = c["chains"][k]
                chains.append([(int(c["seeds"]["rbeg"][c["seed_off"][r] + i]), int(c["seeds"]["qbeg"][c["seed_off"][r] + i]), int(c["seeds"]["len"][c["seed_off"][r] + i]))
                               for i in c["cs"][int(x["first_seed"]):int(x["first_seed"]) + int(x["n"])]])
            reads.append(Rd("%s read %d" % (tag, r), seqs[r], chains, frac=[float(c["chains"]["frac_rep"][k]) for k in range(int(c["chain_off"][r]), int(c["chain_off"][r + 1]))]))
        part = Part(wd, reads)
        refs, t = part_reference(part)
        n_od = sum(1 for x in refs if x[0] is None)
        COUNTS["realistic_" + tag] = dict(reads=len(reads), chains=sum(len(r.chains) for r in reads), regions_before=sum(x[1] for x in refs),
                                          regions_after=sum(len(x[0]) for x in refs if x[0] is not None), order_dependent=n_od, near=t.near(), tally=dict(t.c))
        assert n_od * 20 <= len(reads), (tag, "order-dependent reads above 5 %", n_od, len(reads))
        orows, nb = run_oracle(oracle, part)
        assert nb == [x[1] for x in refs], (tag, "regions before the dedup, oracle against reference")
        hold(orows, refs, part, "the oracle", tag)
        _REAL[tag] = (part, refs, orows)
    part, refs, orows = _REAL[tag]
    rows = rows_of(regs)
    per = [rows[int(ro[r]):int(ro[r + 1])] for r in range(len(seqs))]
    hold(per, refs, part, who, tag)
    assert per == orows, (who, tag, "against the oracle")
    rc_ = COUNTS["realistic_" + tag].setdefault("routes_" + who.split()[1], {})
    for rt in route:
        rc_[str(int(rt))] = rc_.get(str(int(rt)), 0) + 1


def test_emu_slice_reads_against_reference(emu_lib, oracle):
    check_realistic(emu_lib, oracle, common.EXAMPLE_FA, "slice", "the emulation build")


def test_emu_repeat_mid_reads_against_reference(emu_lib, oracle, repeat_mid_prefix):
    check_realistic(emu_lib, oracle, repeat_mid_prefix, "repeat_mid", "the emulation build")


@pytest.mark.gpu
def test_gpu_slice_reads_against_reference(gpu_lib, oracle):
    check_realistic(gpu_lib, oracle, common.EXAMPLE_FA, "slice", "the HIP build")


@pytest.mark.gpu
def test_gpu_repeat_mid_reads_against_reference(gpu_lib, oracle, repeat_mid_prefix):
    check_realistic(gpu_lib, oracle, repeat_mid_prefix, "repeat_mid", "the HIP build")


def test_zz_what_the_reference_evaluated():
    """Over every constructed group -- evaluated here unless a test above has done so -- and the realistic sets that ran: reads, regions before and after the
    dedup, routes, near sites, order-dependent reads.  No read is order-dependent outside the group built for them (asserted per group).  Where
    SSG_REGION_COUNTS_OUT names a directory the figures go to region_reference_counts.json there (profiles/region_reference_counts.json is such a file)."""
    for n in GROUP_NAMES:
        group_reference(group(n))
    assert sum(COUNTS[n]["order_dependent"] for n in GROUP_NAMES if n != "order_dependent") == 0
    assert sum(COUNTS[n]["near"] for n in GROUP_NAMES if not group(n).near) == 0
    assert sum(COUNTS[n]["reads"] for n in GROUP_NAMES) >= 300 and sum(COUNTS[n]["regions_before"] for n in GROUP_NAMES) >= 15000
    out = os.environ.get("SSG_REGION_COUNTS_OUT")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "region_reference_counts.json"), "w") as f:
            json.dump(COUNTS, f, indent=1, sort_keys=True)
