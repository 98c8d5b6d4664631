"""The record stage (mem_reg2aln -> bwa_gen_cigar2 -> ksw_global2, NM and MD) against tests/record_reference.py.

Three legs.  (1) The reference against itself: infer_bw and w2 worked by hand, the retry as a list, NM / MD and the text they rebuild, the path count.  (2)
Constructed regions and requests, in groups named after the seams of the device code (csrc/k_aln.h, ssgpu_core.cpp run_reg2aln); every group asserts ON THE
REFERENCE ALONE that its boundary was reached and states the expected route; then the oracle (orc_api_reg2aln), the emulation build and -- `gpu' -- the HIP
build (ssg_dbg_reg2aln: the host function the pipeline's request tail runs) are each held to the reference, every field of ssg_aln_t.  Every part runs three
times: as it is, with SSG_R2A_DPLANE=0 (the wave kernel answers everything with a gap) and with a read of 300 bases added to the batch (the WIDE instance of the
wave kernel answers).  (3) The regions and requests of simulated pairs.

A region is built from an edit script on the forward strand (`=' copy, `X' mismatch, `N', `D' skip reference bases, `I' insert a base that differs from both
neighbours), so its true score is known; `truesc' and the region's `w' are then free dials for w2 and the retry.  Outside the group `ties' every record has
a unique optimum (asserted on the reference's path count)."""
import json
import os

import numpy as np
import pytest

import record_reference as rec
from speedseq_amd import capi

LANE, DP0, DP1, DP2, WAVE = capi.R2A_ROUTE_LANE, capi.R2A_ROUTE_DP0, capi.R2A_ROUTE_DP1, capi.R2A_ROUTE_DP2, capi.R2A_ROUTE_WAVE
EINVAL, EOVERFLOW = -22, -75
R2D_NEG = -16384          # the lane DP's "minus infinity" in its 16-bit cells (csrc/k_aln.h)


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
def pac_of(text):
    l = len(text)
    c = np.zeros((l // 4 + 1) * 4, dtype=np.uint8)
    c[:l] = text
    c = c.reshape(-1, 4)
    return (c[:, 0] << 6 | c[:, 1] << 4 | c[:, 2] << 2 | c[:, 3]).astype(np.uint8)


class World:
    def __init__(self, text, ctg_len):
        self.text, self.l_pac, self.pac, self.ctg_len = [int(c) for c in text], len(text), pac_of(text), list(ctg_len)
        assert sum(ctg_len) == self.l_pac
        self.ctg_off = [int(x) for x in np.concatenate([[0], np.cumsum(ctg_len)[:-1]])]
        self.ref = rec.Ref(self.pac, self.l_pac, self.ctg_off, self.ctg_len)


_WORLDS = {}


def world(name="two"):
    if name not in _WORLDS:
        if name == "two":
            _WORLDS[name] = World(np.random.RandomState(5).randint(0, 4, 200000).astype(np.uint8), [120000, 80000])
        elif name == "rep":      # homopolymers and tandem repeats inside random text
            t = np.random.RandomState(6).randint(0, 4, 6000).astype(np.uint8)
            t[1000:1010] = 0
            t[999], t[1010] = 1, 2
            t[2000:2018] = [1, 0, 2] * 6
            t[1999], t[2018] = 3, 3
            t[3000:3012] = [0, 3] * 6
            t[2999], t[3012] = 1, 1
            t[1100:1110] = 3
            t[1099], t[1110] = 0, 1
            t[3500:3507] = [1, 1, 0, 1, 0, 0, 1]          # (two small windows for the group `ties': see there)
            t[3600:3606] = [0, 2, 0, 0, 1, 0]
            _WORLDS[name] = World(t, [4000, 2000])
    return _WORLDS[name]


def rnd(n, seed):
    return [int(x) for x in np.random.RandomState(seed).randint(0, 4, n)]


def revcomp(codes):
    return [4 if c > 3 else 3 - c for c in reversed(codes)]


def build(wd, p, script):
    """the forward-strand piece of a script from forward position p: (codes, reference bases spanned)"""
    t, out, p0 = wd.text, [], p
    for op, n in script:
        if op == "=":
            out += t[p:p + n]; p += n
        elif op == "X":
            out += [(c + 1) % 4 for c in t[p:p + n]]; p += n
        elif op == "N":
            out += [4] * n; p += n
        elif op == "D":
            p += n
        elif op == "I":
            out += [min(c for c in range(4) if c != t[p - 1] and c != t[p])] * n
        elif op == "J":           # (an insertion that repeats the next base: for the group `ties')
            out += [t[p]] * n
        else:
            raise ValueError(op)
    return out, p - p0


def slides(wd, p, script):
    """True where a deletion of the script could move by a base (a deleted stretch that begins like what follows it, or ends like what precedes it)"""
    t = wd.text
    for op, n in script:
        if op == "D" and p > 0 and p + n < len(t) and (t[p] == t[p + n] or t[p - 1] == t[p + n - 1]):
            return True
        if op in "=XND":
            p += n
    return False


def script_score(opt, script):
    o = rec.opt_from(**opt)
    s = 0
    for op, n in script:
        s += n * o["a"] if op == "=" else -n * o["b"] if op == "X" else -n if op == "N" else -(o["o_del"] + n * o["e_del"]) if op == "D" else -(o["o_ins"] + n * o["e_ins"])   # (I and J)
    return s


class Part:
    """one call of the entry: a world, options, reads, regions, requests; overflow = the device error code where the call must return SSG_EOVERFLOW"""

    def __init__(self, wd, opt=None, overflow=0, rule="exact", oracle=True):
        self.wd, self.opt, self.overflow, self.rule, self.oracle = wd, dict(opt or {}), overflow, rule, oracle
        self.reads, self.regs, self.reqs = [], [], []

    def add(self, tag, p, script, rev=False, lc=0, rc=0, truesc=None, w=None, want=None, route=None, tie=False, kind=0, owner=0, flag=0, mapq=37, secondary=-1, place=True):
        """a read, its region and one request; lc / rc: clipped bases left / right on the forward strand; want(r): what the group claims of the reference's result"""
        wd = self.wd
        while place and slides(wd, p, script):
            p += 1
        piece, span = build(wd, p, script)
        k = len(self.reads)
        fwd = rnd(lc, 1000 + k) + piece + rnd(rc, 2000 + k)
        L = wd.l_pac
        if rev:
            read, rb, re, qb = revcomp(fwd), 2 * L - (p + span), 2 * L - p, rc
        else:
            read, rb, re, qb = fwd, p, p + span, lc
        sc = script_score(self.opt, script)
        reg = dict(rb=rb, re=re, qb=qb, qe=qb + len(piece), rid=wd.ref.rid_of(rb), score=max(sc, 0), truesc=sc if truesc is None else truesc, sub=k % 7, csub=(k * 3) % 5,
                   w=rec.opt_from(**self.opt)["w"] if w is None else w, secondary=secondary, read=k)
        self.reads.append(read); self.regs.append(reg)
        self.req(tag, k, len(self.regs) - 1, kind=kind, owner=owner, flag=flag, mapq=mapq, want=want, route=route, tie=tie)
        self.reqs[-1]["p"] = p
        return self.reqs[-1]

    def add_raw(self, tag, piece, p, span, rev=False, truesc=0, w=None, **kw):
        """a read given as its forward-strand codes against forward bases [p, p + span)"""
        L, k = self.wd.l_pac, len(self.reads)
        rb, re = (2 * L - (p + span), 2 * L - p) if rev else (p, p + span)
        self.reads.append(revcomp(piece) if rev else list(piece))
        self.regs.append(dict(rb=rb, re=re, qb=0, qe=len(piece), rid=self.wd.ref.rid_of(rb), score=max(truesc, 0), truesc=truesc, sub=0, csub=0,
                              w=rec.opt_from(**self.opt)["w"] if w is None else w, secondary=-1, read=k))
        self.req(tag, k, len(self.regs) - 1, **kw)
        self.reqs[-1]["p"] = p

    def req(self, tag, read, reg, kind=0, owner=0, flag=0, mapq=37, want=None, route=None, tie=False):
        self.reqs.append(dict(tag=tag, read=read, reg=reg, kind=kind, owner=owner, flag=flag, mapq=mapq, want=want, route=route, tie=tie))

    def packed(self, extra_wide=False):
        reads, regs, reqs = list(self.reads), list(self.regs), list(self.reqs)
        if extra_wide:        # a read of 300 bases that matches the reference: the batch's longest read selects the wave kernel's instance
            reads.append(self.wd.text[50000 % (self.wd.l_pac - 400):][:300])
            p = 50000 % (self.wd.l_pac - 400)
            regs.append(dict(rb=p, re=p + 300, qb=0, qe=300, rid=self.wd.ref.rid_of(p), score=300, truesc=300 * rec.opt_from(**self.opt)["a"], sub=0, csub=0, w=100, secondary=-1))
            reqs.append(dict(read=len(reads) - 1, reg=len(regs) - 1, kind=0, owner=0, flag=0, mapq=1))
        seq = np.array([c for r in reads for c in r], dtype=np.uint8)
        off = np.zeros(len(reads) + 1, dtype=np.int64); off[1:] = np.cumsum([len(r) for r in reads])
        rg = np.zeros(len(regs), capi.ALNREG_DT)
        for k, r in enumerate(regs):
            for f in ("rb", "re", "qb", "qe", "rid", "score", "truesc", "sub", "csub", "w", "secondary"):
                rg[f][k] = r[f]
            rg["secondary_all"][k] = -1; rg["seedcov"][k] = 7; rg["sub_n"][k] = 1; rg["seedlen0"][k] = 19; rg["frac_rep"][k] = 0.25; rg["hash"][k] = 12345 + k
        rq = np.zeros(len(reqs), capi.ALNREQ_DT)
        for k, r in enumerate(reqs):
            for f in ("read", "reg", "kind", "owner", "flag", "mapq"):
                rq[f][k] = r[f]
        return dict(seq=seq, off=off, regs=rg, req=rq, max_len=max(len(r) for r in reads))

    def lib_opt(self, lib):
        o = lib.opt_init()
        for k, v in self.opt.items():
            o[k] = v
        if "a" in self.opt or "b" in self.opt:
            a, b = int(o["a"][0]), int(o["b"][0])
            o["mat"][0] = np.array([[(a if i == j else -b) if i < 4 and j < 4 else -1 for j in range(5)] for i in range(5)], dtype=np.int8).reshape(-1)
        return o

    def orc_opt(self, oracle):
        o = rec.opt_from(**self.opt)
        h = oracle.opt_scores(o["a"], o["b"], o["o_del"], o["e_del"], o["o_ins"], o["e_ins"])
        return oracle.opt_regions(h, o["w"], 100, 5, 5, 10000, 0.95)


class Group:
    def __init__(self, name, aim, parts, ties=False):
        self.name, self.aim, self.parts, self.ties = name, aim, parts, ties


def row_of_ref(r):
    return (r["pos"], r["rid"], r["flag"], r["mapq"], r["NM"], r["score"], r["sub"], r["n_cigar"], r["is_rev"], r["l_md"], r["reg_idx"], r["xa_cnt"], r["kind"] or 0,
            tuple(r["cigar"]), r["md"].encode())


def rows_of(alns):
    out = []
    for a in alns:
        n = min(int(a["n_cigar"]), 64)
        md = bytes(a["md"]).ljust(320, b"\0")          # MD is a C string: l_md characters and a terminator; what lies behind it (an earlier round's text) is nobody's
        assert 0 <= int(a["l_md"]) < 320 and md[int(a["l_md"])] == 0, (int(a["l_md"]), md)
        out.append((int(a["pos"]), int(a["rid"]), int(a["flag"]), int(a["mapq"]), int(a["NM"]), int(a["score"]), int(a["sub"]), int(a["n_cigar"]), int(a["is_rev"]), int(a["l_md"]),
                    int(a["reg_idx"]), int(a["xa_cnt"]), int(a["_pad"]), tuple(int(c) for c in a["cigar"][:n]), md[:int(a["l_md"])]))
    return out


ROW_FIELDS = ("pos", "rid", "flag", "mapq", "NM", "score", "sub", "n_cigar", "is_rev", "l_md", "reg_idx", "xa_cnt", "kind", "cigar", "md")


def expected_route(r, max_len, dplane):
    """the route of a record, from the reference's rounds alone: the first band's class, handed on when the retry goes on or the window exceeds the lane DP's rows"""
    if r["pos"] < 0 and r["rid"] < 0:
        return 0
    if r["rounds"][0][1] is None:
        return LANE
    if not dplane:
        return WAVE
    b0 = r["rounds"][0][1]
    cls = DP0 if b0 <= 8 else DP1 if b0 <= 16 else DP2 if b0 <= 32 else 0
    if not cls:
        return WAVE
    return cls | (WAVE if len(r["rounds"]) > 1 or r["tlen"] > max_len + 32 else 0)


_REFS, COUNTS = {}, {}


def part_reference(part):
    out = []
    o = rec.opt_from(**part.opt)
    for q in part.reqs:
        reg = part.regs[q["reg"]] if q["reg"] >= 0 else None
        r = rec.record(o, part.wd.ref, part.reads[q["read"]], reg, q)
        r.update(qlen=reg["qe"] - reg["qb"] if reg else 0, truesc=reg["truesc"] if reg else 0, tlen=reg["re"] - reg["rb"] if reg else 0, rb=reg["rb"] if reg else -1, re=reg["re"] if reg else -1, p=q.get("p"))
        out.append(r)
    return out


def group_reference(g):
    """every part of the group through the reference, once; what the group claims is asserted here, on the reference alone"""
    if g.name not in _REFS:
        res, cnt = [], dict(records=0, forced=0, gap_free=0, rounds={}, bands={}, routes={}, overflow_parts=0)
        for part in g.parts:
            refs = part_reference(part)
            res.append(refs)
            ml = max(len(r) for r in part.reads)
            for q, r in zip(part.reqs, refs):
                ctx = (g.name, q["tag"])
                if q["want"] is not None:
                    assert q["want"](r), (ctx, "the boundary this record was built for was not reached", {k: r.get(k) for k in ("rounds", "band", "n_paths", "cigar", "md", "lo_first", "pos")})
                if q["reg"] >= 0:
                    assert r["forced"] or q["tie"], (ctx, "more than one optimal path outside the group `ties'", r["n_paths"], r["cigar"])
                    assert not (q["tie"] and not g.ties), ctx
                er = expected_route(r, ml, True)
                if q["route"] is not None and part.rule == "exact":
                    assert er == q["route"], (ctx, "the route the reference implies is not the one the group states", er, q["route"], r.get("rounds"))
                cnt["records"] += 1; cnt["forced"] += bool(r.get("forced")); cnt["gap_free"] += bool(r.get("gap_free"))
                if "rounds" in r:
                    cnt["rounds"][str(len(r["rounds"]))] = cnt["rounds"].get(str(len(r["rounds"])), 0) + 1
                    cnt["bands"][str(r["band"])] = cnt["bands"].get(str(r["band"]), 0) + 1
                cnt["routes"][str(er)] = cnt["routes"].get(str(er), 0) + 1
            cnt["overflow_parts"] += bool(part.overflow)
        COUNTS[g.name] = cnt
        _REFS[g.name] = res
    return _REFS[g.name]


def hold(rows, refs, part, who, gname):
    for q, got, r in zip(part.reqs, rows, refs):
        want = row_of_ref(r)
        if got != want:
            bad = [f for f, a, b in zip(ROW_FIELDS, got, want) if a != b]
            raise AssertionError("%s: %s, record `%s': fields %s differ: got %s, the reference has %s (rounds %s)" % (gname, who, q["tag"], bad, [got[ROW_FIELDS.index(f)] for f in bad],
                                                                                                                [want[ROW_FIELDS.index(f)] for f in bad], r.get("rounds")))


def check_group_oracle(g, oracle):
    for part, refs in zip(g.parts, group_reference(g)):
        if not part.oracle:
            continue
        p = part.packed()
        alns, over = oracle.reg2aln(part.wd.pac, part.wd.l_pac, part.wd.ctg_off, part.wd.ctg_len, p["seq"], p["off"], p["regs"], p["req"], opt=part.orc_opt(oracle))
        if part.overflow in (6, 7):
            continue              # (upstream has no capacity; what it makes beyond ours is cut to the layout and not compared)
        assert not over.any()
        hold(rows_of(alns), refs, part, "the oracle", g.name)


def check_group_library(g, lib, who, monkeypatch):
    all_refs = group_reference(g)
    routes = COUNTS[g.name].setdefault("routes_" + who.split()[1], {})
    for part, refs in zip(g.parts, all_refs):
        for mode in ("plain", "no lane DP", "wide"):
            monkeypatch.setenv("SSG_R2A_DPLANE", "0" if mode == "no lane DP" else "1")
            p = part.packed(extra_wide=mode == "wide")
            rc, alns, route, err = lib.dbg_reg2aln(part.lib_opt(lib), part.wd.pac, part.wd.l_pac, part.wd.ctg_off, part.wd.ctg_len, p["seq"], p["off"], p["regs"], p["req"])
            ctx = (g.name, who, mode)
            if part.overflow:
                # (code 5 is the wave kernel's slab: the lane DP never has it; 6 and 7 come from every kernel that makes such a record)
                assert (rc, err) == (EOVERFLOW, part.overflow), (ctx, "a record beyond a capacity must end the call with SSG_EOVERFLOW", rc, err)
                continue
            assert (rc, err) == (0, 0), (ctx, rc, err)
            n = len(part.reqs)
            hold(rows_of(alns[:n]), refs, part, "%s (%s)" % (who, mode), g.name)
            for q, r, rt in zip(part.reqs, refs, route[:n]):
                rt = int(rt)
                if mode == "plain":
                    routes[str(rt)] = routes.get(str(rt), 0) + 1
                if part.rule == "exact":
                    er = expected_route(r, p["max_len"], mode != "no lane DP")
                    assert rt == er, (ctx, q["tag"], "route", rt, er, r.get("rounds"))
                elif q["reg"] >= 0 and not r["gap_free"] and beyond_lane_cells(r, rec.opt_from(**part.opt)):
                    assert rt & WAVE, (ctx, q["tag"], "a record whose cells leave the lane DP's range was not sent to the wave kernel", rt, r["lo_first"])
    monkeypatch.delenv("SSG_R2A_DPLANE", raising=False)


def beyond_lane_cells(r, o):
    """from the reference's extremes of the first band: a value of a reachable cell at or below what derives from the lane DP's minus infinity (at most
    R2D_NEG + a), or outside 16 bits"""
    return r["lo_first"] <= R2D_NEG + o["a"] or r["lo_first"] < -32768 or r["hi_first"] > 32767


# ------------------------------------------------------------------------------------------------------------------------------
# the groups
# ------------------------------------------------------------------------------------------------------------------------------
def mm(n, at, total):
    """a script of `total' columns with mismatches at the given columns"""
    s, k = [], 0
    for a in sorted(at):
        if a > k:
            s.append(("=", a - k))
        s.append(("X", 1)); k = a + 1
    if total > k:
        s.append(("=", total - k))
    return s


def g_gap_free_edge():
    wd = world()
    parts = []
    p = Part(wd)                     # 2 (o + e - a) = 12; a mismatch costs a + b = 5
    p.add("two mismatches: 10 < 12", 1000, mm(2, [10, 30], 50), want=lambda r: r["gap_free"] and 50 * 1 - r["truesc"] == 10 < 2 * (6 + 1 - 1), route=LANE)
    p.add("three mismatches: 15 >= 12", 1100, mm(3, [10, 30, 40], 50), want=lambda r: not r["gap_free"] and r["rounds"][0][0] > 0 and 50 * 1 - r["truesc"] == 15 >= 2 * (6 + 1 - 1), route=DP1)
    p.add("truesc one below the edge", 1200, [("=", 50)], truesc=50 - 11, want=lambda r: r["gap_free"], route=LANE)
    p.add("truesc exactly at the edge", 1200, [("=", 50)], truesc=50 - 12, want=lambda r: not r["gap_free"] and r["band"] == 8, route=DP0)
    p.add("two mismatches, reverse strand", 1300, mm(2, [0, 49], 50), rev=True, want=lambda r: r["gap_free"] and r["md"][0] == "0" and r["md"][-1] == "0", route=LANE)
    parts.append(p)
    p = Part(wd, dict(b=5))          # a mismatch costs 6: two of them sit exactly on 12
    p.add("-B 5, two mismatches: 12 == 12", 1000, mm(2, [10, 30], 50), want=lambda r: not r["gap_free"], route=DP0)
    p.add("-B 5, one mismatch", 1100, mm(1, [10], 50), want=lambda r: r["gap_free"], route=LANE)
    parts.append(p)
    o = dict(o_del=7, e_del=2, o_ins=5, e_ins=1)      # 2 (o + e - a): 16 for a deletion, 10 for an insertion
    p = Part(wd, o)
    a = rec.opt_from(**o)
    bw = lambda ts: (rec.infer_bw(50, 50, ts, 1, a["o_del"], a["e_del"]), rec.infer_bw(50, 50, ts, 1, a["o_ins"], a["e_ins"]))
    assert bw(41) == (0, 0) and bw(40) == (0, 7) and bw(35) == (0, 12) and bw(34) == (6, 13)
    p.add("unequal gap costs, both zero", 1000, [("=", 50)], truesc=41, want=lambda r: r["gap_free"], route=LANE)
    p.add("unequal gap costs, the insertion's decides", 1000, [("=", 50)], truesc=40, want=lambda r: r["rounds"][0][0] == 7 and r["band"] == 7, route=DP0)
    p.add("unequal gap costs, both above zero", 1000, [("=", 50)], truesc=34, want=lambda r: r["rounds"][0][0] == 13, route=DP1)
    parts.append(p)
    return Group("gap_free_edge", "l a - truesc one below and exactly at 2 (o + e - a); -B 5 with two mismatches on it; unequal gap costs", parts)


def g_band_classes():
    wd = world()
    p = Part(wd)
    # at default scoring and equal lengths the smallest w2 above 0 is 8 (l a - truesc = 12): smaller ones come through the region's w, which caps w2 where it
    # is above opt.w -- two parts with -w 2 and -w 1
    p3, p1 = Part(wd, dict(w=2)), Part(wd, dict(w=1))
    cls = lambda b: DP0 if b <= 8 else DP1 if b <= 16 else DP2 if b <= 32 else WAVE
    o = rec.opt_from()
    for k, B in enumerate((3, 8, 9, 16, 17, 32, 33)):
        at = 3000 + 400 * k
        # through w2: equal lengths, 150 columns (half the query pays for a band of 35), truesc the dial: w2 = 150 - truesc - 4
        if B == 3:
            p3.add("band 3 through w2", at, mm(1, [70], 150), truesc=150 - 12, w=3, route=DP0, want=lambda r: r["band"] == 3 and r["rounds"][0][0] == 3)
        else:
            p.add("band %d through w2" % B, at, mm(1, [70], 150), truesc=150 - 4 - B, route=cls(B),
                  want=lambda r, B=B: r["band"] == B and r["rounds"][0][0] == B and rec.gen_band(o, 150, 150, 1000) == 35)
        # through |difference| + 3: a deletion of B - 3 bases (for B = 3: none, and a w2 of 1 through the region's w)
        d = B - 3
        if d == 0:
            p1.add("band 3 through |difference| + 3", at + 200, mm(1, [20], 150), truesc=150 - 12, w=1, route=DP0, want=lambda r: r["band"] == 3 and r["rounds"][0][0] == 1)
        else:
            p.add("band %d through |difference| + 3" % B, at + 200, [("=", 75), ("D", d), ("=", 75)], route=cls(B),
                  want=lambda r, B=B, d=d: r["band"] == B == d + 3 and r["rounds"][0][0] < B)
        # through the cap (max_gap + |difference| + 1) >> 1: a query of 4 B + 7 bases pays for a gap of 2 B, w2 is B + 5 through truesc
        lq = 4 * B + 7
        p.add("band %d through the cap, query of %d" % (B, lq), at + 600 - lq, mm(1, [lq // 2], lq), truesc=lq - 4 - (B + 5), route=cls(B),
              want=lambda r, B=B, lq=lq: r["band"] == B and r["rounds"][0][0] == B + 5 and rec.gen_band(o, lq, lq, 1000) == B)
    return Group("band_classes", "final bands 3, 8, 9, 16, 17, 32, 33, each through w2, through |difference| + 3 and through the cap", [p, p3, p1])


def band_widths(qlen, tlen, w):
    return set((min(qlen, i + w + 1) - max(0, i - w)) % 8 for i in range(tlen))


def g_ring_and_words():
    wd = world()
    p, p3 = Part(wd), Part(wd, dict(w=2))
    for k, lq in enumerate((1, 2, 7, 8, 9, 15, 16, 17)):
        at = 8000 + 100 * k
        # the query against a window one base longer at its end: an end deletion, squeezed; and with a deletion of 2 inside where there is room
        p.add("query of %d, window one longer" % lq, at, [("=", lq), ("D", 1)], want=lambda r, lq=lq: r["band"] == 4 and r["cigar"] == [lq << 4], route=DP0)
        if lq >= 7:
            p.add("query of %d, deletion of 2" % lq, at + 40, [("=", lq // 2), ("D", 2), ("=", lq - lq // 2)], want=lambda r: r["band"] == 5 and r["n_cigar"] == 3, route=DP0)
        # equal lengths with a band through truesc (w2 = 8, and a short query pays for a band of 3 at most): the DP runs on a window of lq rows
        if lq >= 2:
            p.add("query of %d, equal lengths" % lq, at + 70, mm(1, [lq - 1], lq), truesc=lq - 12, want=lambda r: r["band"] == 3 and r["rounds"][0][0] == 8, route=DP0)
    p.add("window of one base, query of 1", 9000, [("X", 1)], truesc=-11, want=lambda r: r["tlen"] == 1 and not r["gap_free"] and r["md"] == "0%s0" % "ACGT"[wd.text[9000]], route=DP0)
    p.add("window of one base, query of 2", 9010, [("=", 1), ("I", 1)], want=lambda r: r["tlen"] == 1 and r["cigar"] == [1 << 4, 1 << 4 | 1], route=DP0)
    # 2 w, 2 w + 1, 2 w + 2 columns: band 3 (through truesc) and bands 8, 16, 32, the widest of each class (a deletion of w - 3); the row is 2 w + 1 cells wide once, then clipped by the query's end
    for w, d, route in ((3, 0, DP0), (8, 5, DP0), (16, 13, DP1), (32, 29, DP2)):
        for lq in (2 * w, 2 * w + 1, 2 * w + 2):
            sc = [("=", lq // 2), ("D", d), ("=", lq - lq // 2)] if d else mm(1, [lq // 2], lq)
            p.add("query of %d = 2 w + %d, band %d" % (lq, lq - 2 * w, w), 9100 + 50 * lq + d, sc, truesc=None if d else lq - 12,
                  want=lambda r, w=w, lq=lq: r["band"] == w and r["qlen"] == lq, route=route)
    # long queries in the narrowest class: the ring of 2 x 8 + 2 columns wraps (150 columns), and so does the first slot (windows beyond 18 rows)
    p3.add("150 columns in band 3: the ring wraps", 9900, mm(2, [3, 100], 150), truesc=150 - 12, w=3, want=lambda r: r["band"] == 3 and r["tlen"] > 18, route=DP0)
    p.add("150 columns in band 8", 10100, [("=", 70), ("D", 5), ("=", 80)], want=lambda r: r["band"] == 8 and r["tlen"] > 18, route=DP0)
    # a path along the band's edges in the widest band of each class, where every slot of the ring is live: a deletion and an insertion of wmax bases (the path runs
    # wmax below the diagonal, in the row's first column) and the other way round (its last column); w2 is opt.w << 2 through the region's w
    edge_parts = []
    for wmax, route in ((8, DP0), (16, DP1), (32, DP2)):
        pe = Part(wd, dict(w=wmax >> 2))
        n = 150
        pe.add("the lower edge of band %d" % wmax, 10500, indel_pairs(n, [wmax]), w=wmax, route=route,
               want=lambda r, wmax=wmax, n=n: r["band"] == wmax and r["rounds"] == [(wmax, wmax, nat([wmax], n))] and r["n_cigar"] == 5)
        up = [("=", 20), ("I", wmax), ("=", 20), ("D", wmax), ("=", n - 40 - wmax)]
        pe.add("the upper edge of band %d" % wmax, 11000, up, w=wmax, rev=True, route=route,
               want=lambda r, wmax=wmax, n=n: r["band"] == wmax and r["rounds"] == [(wmax, wmax, nat([wmax], n))] and r["n_cigar"] == 5)
        edge_parts.append(pe)
    g = Group("ring_and_words", "queries of 1 .. 17 and 2 w .. 2 w + 2 bases, a window of one base, rows whose width is 0, 1 and 7 above a multiple of 8, a ring that wraps, "
              "paths along both edges of bands 8, 16 and 32", [p, p3] + edge_parts)
    g.widths = lambda refs: set().union(*[band_widths(len(p.reads[q["read"]]), r["tlen"], r["band"]) for q, r in zip(p.reqs, refs) if r.get("band")])
    return g


def indel_pairs(n, gaps):
    """n columns on either side: for every gap a deletion and an insertion of that many bases 20 columns apart -- equal lengths, and a band of `gap' to follow each"""
    s, used = [], 0
    for g_ in gaps:
        s += [("=", 20), ("D", g_), ("=", 20), ("I", g_)]
        used += 40 + g_
    return s + [("=", n - used)]


def nat(gaps, n=150):
    return n - sum(gaps) - sum(2 * (6 + g_) for g_ in gaps)


def g_retry():
    wd = world()
    parts = []
    # opt.w = 5: the w2 of the true score is above it and so capped by the region's w; 2 -> 4 -> 8 (-> 16), bands 3, 4, 8
    p = Part(wd, dict(w=5))
    ws = lambda r: [x[0] for x in r["rounds"]]
    sc = lambda r: [x[2] for x in r["rounds"]]
    p.add("gaps of 4: doubles once", 20000, indel_pairs(150, [4]), w=2, route=DP0 | WAVE, want=lambda r: ws(r) == [2, 4] and sc(r)[0] < nat([4]) - 1 and sc(r)[1] == nat([4]))
    p.add("gaps of 4 and 7: doubles twice", 20400, indel_pairs(150, [4, 7]), w=2, route=DP0 | WAVE,
          want=lambda r: ws(r) == [2, 4, 8] and sc(r)[0] < sc(r)[1] < sc(r)[2] == nat([4, 7]))
    p.add("truesc beyond every band: three rounds and no more", 20800, indel_pairs(150, [4, 7]), w=2, truesc=nat([4, 7]) + 5, route=DP0 | WAVE,
          want=lambda r: ws(r) == [2, 4, 8] and sc(r)[0] < sc(r)[1] < sc(r)[2] == nat([4, 7]) < r["truesc"] - 1)
    p.add("the region's w above opt.w: w2 capped at opt.w << 2", 21200, indel_pairs(150, [12]), w=50, route=DP2,
          want=lambda r: ws(r) == [20] and r["band"] == 20 and sc(r)[0] == nat([12]))
    parts.append(p)
    # stops on an equal score: mismatches alone, and a truesc no band can earn
    p = Part(wd)
    p.add("stops on an equal score", 22000, mm(3, [20, 70, 120], 150), truesc=138, route=DP0 | WAVE,
          want=lambda r: [x[0] for x in r["rounds"]] == [8, 16] and r["rounds"][0][2] == r["rounds"][1][2] == 135)
    p.add("score within one match of truesc: no second round", 22400, mm(3, [20, 70, 120], 150), truesc=136, route=DP1, want=lambda r: len(r["rounds"]) == 1 and r["rounds"][0][2] == 135)
    p.add("score one further from truesc: a second round", 22400, mm(3, [20, 70, 120], 150), truesc=137, route=DP1 | WAVE, want=lambda r: len(r["rounds"]) == 2 and r["rounds"][0][2] == 135)
    parts.append(p)
    # stops on opt.w << 2 = 8: 3 -> 6 -> 8
    p = Part(wd, dict(w=2))
    p.add("stops on opt.w << 2", 23000, indel_pairs(150, [4, 7]), w=3, truesc=nat([4, 7]) + 5, route=DP0 | WAVE,
          want=lambda r: [x[0] for x in r["rounds"]] == [3, 6, 8] and r["rounds"][0][2] < r["rounds"][1][2] < r["rounds"][2][2] == nat([4, 7]) < r["truesc"] - 1)
    p.add("begins on opt.w << 2: the lane DP keeps it whatever the score", 23400, indel_pairs(150, [7]), w=8, truesc=nat([7]) + 5, route=DP0,
          want=lambda r: [x[0] for x in r["rounds"]] == [8] and r["rounds"][0][2] == nat([7]) < r["truesc"] - 1)
    parts.append(p)
    return Group("retry", "truesc above what the first band earns: doubles once, twice, three rounds; stops on an equal score, on opt.w << 2; the region's w below and above opt.w", parts)


def g_wave_columns():
    wd = world()
    parts = []
    for lens in ((63, 64, 127, 128, 191, 192, 255), (256, 309, 310)):
        p = Part(wd)
        for k, lq in enumerate(lens):
            p.add("query of %d, deletion of 31" % lq, 30000 + 700 * k, [("=", lq // 2), ("D", 31), ("=", lq - lq // 2)], rev=bool(k & 1), route=WAVE,
                  want=lambda r: r["band"] == 34 and r["n_cigar"] == 3)
            p.add("query of %d, insertion of 30" % lq, 30350 + 700 * k, [("=", lq // 3), ("I", 30), ("=", lq - 30 - lq // 3)], route=WAVE, want=lambda r: r["band"] == 33 and r["n_cigar"] == 3)
        parts.append(p)
    # windows of 1024 and 1025 bases: the LDS window and the global one.  The deletion lies at an end: in the middle its letters would fill MD beyond its capacity
    p = Part(wd, dict(w=1000))
    for span in (1024, 1025):
        p.add("window of %d bases, the deletion last" % span, 40000, [("=", 150), ("D", span - 150)], w=1000, route=WAVE,
              want=lambda r, span=span: r["tlen"] == span and r["cigar"] == [150 << 4] and r["pos"] == r["p"] and r["md"] == "150")
        p.add("window of %d bases, the deletion first" % span, 42000, [("D", span - 150), ("=", 150)], w=1000, rev=True, route=WAVE,
              want=lambda r, span=span: r["tlen"] == span and r["cigar"] == [150 << 4] and r["pos"] == r["p"] + span - 150)
    parts.append(p)
    return Group("wave_columns", "queries of 63 .. 310 bases in bands beyond 32; windows of 1024 and 1025 bases", parts)


def g_end_gaps():
    wd = world()
    p = Part(wd)
    for rev in (False, True):
        for lc, rc in ((0, 0), (4, 9)):
            t = "%s%s" % (", reverse" if rev else "", ", clips" if lc else "")
            nclip = 2 if lc else 0
            p.add("a deletion first" + t, 50000, [("D", 5), ("=", 60)], rev=rev, lc=lc, rc=rc, route=DP0,
                  want=lambda r, nclip=nclip: r["n_cigar"] == 1 + nclip and r["pos"] == r["p"] + 5 and r["md"] == "60" and r["NM"] == 0 and r["raw_n_cigar"] == 2)
            p.add("a deletion last" + t, 50200, [("=", 60), ("D", 5)], rev=rev, lc=lc, rc=rc, route=DP0,
                  want=lambda r, nclip=nclip: r["n_cigar"] == 1 + nclip and r["pos"] == r["p"] and r["md"] == "60" and r["raw_n_cigar"] == 2)
            p.add("a deletion first and last" + t, 50400, [("D", 5), ("=", 60), ("D", 4)], rev=rev, lc=lc, rc=rc, route=DP2,
                  want=lambda r, nclip=nclip: r["n_cigar"] == 2 + nclip and r["pos"] == r["p"] + 5 and r["raw_n_cigar"] == 3 and r["cigar"][-1 - (1 if nclip else 0)] == (4 << 4 | 2)
                  and r["NM"] == 0 and r["md"] == "60")
            p.add("an insertion first" + t, 50600, [("I", 3), ("=", 60)], rev=rev, lc=lc, rc=rc, route=DP0,
                  want=lambda r, nclip=nclip: r["n_cigar"] == 2 + nclip and r["pos"] == r["p"] and r["NM"] == 3 and r["cigar"][1 if nclip else 0] == (3 << 4 | 1))
            p.add("an insertion last" + t, 50800, [("=", 60), ("I", 3)], rev=rev, lc=lc, rc=rc, route=DP0,
                  want=lambda r, nclip=nclip: r["n_cigar"] == 2 + nclip and r["NM"] == 3 and r["cigar"][-1 - (1 if nclip else 0)] == (3 << 4 | 1))
    # a leading deletion that carries POS across a contig's start: rid is the contig of the final POS.  No region of the pipeline looks like this (a chain's window is
    # cut to its contig), and upstream asserts that the contig has not changed: the oracle, which keeps that assertion, is not asked
    c1 = wd.ctg_off[1]
    px = Part(wd, oracle=False)
    for rev in (False, True):
        px.add("a leading deletion across a contig's start" + (", reverse" if rev else ""), c1 - 5, [("D", 5), ("=", 60)], rev=rev, place=False, route=DP0,
               want=lambda r: (r["rid"], r["pos"]) == (1, 0) and r["rb" if r["rb"] < wd.l_pac else "re"] in (c1 - 5, 2 * wd.l_pac - (c1 - 5)) and r["n_cigar"] == 1)
    return Group("end_gaps", "a deletion first, last and both (one is removed, POS moves with the first); an insertion first and last (kept); both strands, with clips; "
                 "POS across a contig's start", [p, px])


def g_strands_and_clips():
    wd = world()
    p = Part(wd)
    S = lambda n: n << 4 | 3
    for rev in (False, True):
        for lc, rc in ((0, 0), (7, 0), (0, 11), (7, 11)):
            want_gf = lambda r, lc=lc, rc=rc: r["cigar"] == ([S(lc)] if lc else []) + [50 << 4] + ([S(rc)] if rc else []) and r["is_rev"] == int(r["rb"] >= wd.l_pac)
            p.add("clips %d / %d%s, gap-free" % (lc, rc, ", reverse" if rev else ""), 60000, mm(1, [5], 50), rev=rev, lc=lc, rc=rc, want=want_gf, route=LANE)
            p.add("clips %d / %d%s, a deletion" % (lc, rc, ", reverse" if rev else ""), 60300, [("=", 20), ("D", 3), ("=", 30)], rev=rev, lc=lc, rc=rc, route=DP0,
                  want=lambda r, lc=lc, rc=rc: r["cigar"] == ([S(lc)] if lc else []) + [20 << 4, 3 << 4 | 2, 30 << 4] + ([S(rc)] if rc else []))
    # XA-kind requests, several requests on one region, a secondary region, the unmapped request
    q = p.add("main and XA requests on one region", 61000, [("=", 30), ("I", 2), ("=", 30)], lc=3, flag=0x41, mapq=60, owner=0, want=lambda r: r["kind"] == 0 and r["flag"] == 0x41)
    p.req("the same region as an XA entry", q["read"], q["reg"], kind=1, owner=5, flag=0, mapq=0, want=lambda r: r["kind"] == 1 and r["reg_idx"] == 5, route=DP0)
    p.req("the same region again, other flag and mapq", q["read"], q["reg"], kind=0, owner=2, flag=0x881, mapq=3, want=lambda r: r["flag"] == 0x881 and r["mapq"] == 3, route=DP0)
    p.add("a secondary region", 61400, mm(1, [9], 40), secondary=0, flag=0x1, want=lambda r: r["flag"] == 0x101, route=LANE)
    p.req("the unmapped request", q["read"], -1, flag=0x4d, mapq=9, want=lambda r: (r["pos"], r["rid"], r["flag"], r["mapq"], r["n_cigar"], r["reg_idx"]) == (-1, -1, 0x4d, 0, 0, -1), route=0)
    return Group("strands_and_clips", "qb, qe, both, neither; the reverse strand; XA-kind requests; the unmapped request; several requests on one region", [p])


def g_contig_edges():
    wd = world()
    L, c1 = wd.l_pac, wd.ctg_off[1]
    p = Part(wd)
    for tag, at, rev, chk in (("rb = 0", 0, False, lambda r: r["rb"] == 0 and (r["rid"], r["pos"]) == (0, 0)),
                              ("re = l_pac", L - 60, False, lambda r: r["re"] == L and (r["rid"], r["pos"]) == (1, 80000 - 60)),
                              ("rb = l_pac", L - 60, True, lambda r: r["rb"] == L and (r["rid"], r["pos"]) == (1, 80000 - 60)),
                              ("re = 2 l_pac", 0, True, lambda r: r["re"] == 2 * L and (r["rid"], r["pos"]) == (0, 0)),
                              ("the first base of the second contig", c1, False, lambda r: (r["rid"], r["pos"]) == (1, 0)),
                              ("the first base of the second contig, reverse", c1, True, lambda r: (r["rid"], r["pos"]) == (1, 0)),
                              ("the last base of the first contig", c1 - 60, False, lambda r: (r["rid"], r["pos"]) == (0, 120000 - 60)),
                              ("the last base of the first contig, reverse", c1 - 60, True, lambda r: (r["rid"], r["pos"]) == (0, 120000 - 60))):
        # (each script spans 60 reference bases)
        p.add(tag + ", gap-free", at, mm(2, [0, 59], 60), rev=rev, place=False, want=chk, route=LANE)
        k = next(k for k in range(20, 40) if not slides(wd, at, [("=", k), ("D", 2)]))          # (a place where the deletion cannot move)
        p.add(tag + ", a deletion", at, [("=", k), ("D", 2), ("=", 58 - k)], rev=rev, place=False, want=chk, route=DP0)
        p.add(tag + ", an insertion", at, [("=", 31), ("I", 2), ("=", 29)], rev=rev, place=False, want=chk, route=DP0)
    return Group("contig_edges", "rb = 0, re = l_pac, rb = l_pac, re = 2 l_pac; the first and last base of a contig", [p])


def g_query_n():
    wd = world()
    p = Part(wd)
    for rev in (False, True):
        t = ", reverse" if rev else ""
        p.add("an N inside M, gap-free" + t, 70000, [("=", 20), ("N", 1), ("=", 29)], rev=rev, route=LANE, want=lambda r: r["gap_free"] and r["NM"] == 1 and r["md"].count("A") + r["md"].count("C") + r["md"].count("G") + r["md"].count("T") == 1)
        p.add("an N at either end" + t, 70200, [("N", 1), ("=", 48), ("N", 1)], rev=rev, route=LANE, want=lambda r: r["NM"] == 2 and r["md"][0] == "0" and r["md"][-1] == "0")
        p.add("an N inside M, in the DP" + t, 70400, [("=", 20), ("N", 1), ("=", 10), ("D", 2), ("=", 19)], rev=rev, route=DP0, want=lambda r: r["NM"] == 3)
        p.add("an N behind an insertion" + t, 70600, [("=", 20), ("I", 1), ("N", 1), ("=", 28)], rev=rev, route=DP0, want=lambda r: r["NM"] == 2 and r["n_cigar"] == 3)
        p.add("an N at the end of the DP's query" + t, 70800, [("=", 30), ("D", 3), ("=", 19), ("N", 1)], rev=rev, route=DP0, want=lambda r: r["NM"] == 4 and r["md"][-1] == "0")
    return Group("query_n", "an N of the query inside M, next to a gap and at an end: it always mismatches and MD carries the reference's base", [p])


def g_ties():
    wd = world("rep")
    parts = []
    p = Part(wd)
    M, I, D = 0, 1, 2
    for rev in (False, True):
        t = ", reverse" if rev else ""
        # ten A from 1000: a deletion or an insertion of one A lies at the run's first base, whichever base the script took
        p.add("a deletion in a homopolymer" + t, 960, [("=", 45), ("D", 1), ("=", 45)], rev=rev, place=False, tie=True, route=DP0,
              want=lambda r: r["n_paths"] > 1 and r["leftmost"] == 40 and r["cigar"] == [40 << 4, 1 << 4 | D, 50 << 4] and r["md"] == "40^A50")
        p.add("an insertion in a homopolymer" + t, 960, [("=", 45), ("J", 1), ("=", 45)], rev=rev, place=False, tie=True, route=DP0,
              want=lambda r: r["n_paths"] > 1 and r["leftmost"] == 40 and r["cigar"] == [40 << 4, 1 << 4 | I, 50 << 4] and r["md"] == "90")
        # (CAG) x 6 from 2000: a unit deleted in the middle lies at the repeat's start
        p.add("a unit of a tandem repeat deleted" + t, 1960, [("=", 49), ("D", 3), ("=", 40)], rev=rev, place=False, tie=True, route=DP0,
              want=lambda r: r["n_paths"] > 1 and r["leftmost"] == 40 and r["cigar"][:2] == [40 << 4, 3 << 4 | D])
        p.add("two units of (AT) deleted" + t, 2960, [("=", 46), ("D", 4), ("=", 40)], rev=rev, place=False, tie=True, route=DP0,
              want=lambda r: r["n_paths"] > 1 and r["leftmost"] == 40)
    parts.append(p)
    # the restated order for the rest: tied optima that are no single gap, so that nothing but the backtrace's preference (a diagonal step before a deletion before
    # an insertion from the last cell back; "open" where opening and extending tie) stands behind the CIGAR.  Each asserts n_paths > 1 and leftmost is None
    tied = lambda r: r["n_paths"] > 1 and r["leftmost"] is None
    p = Part(wd)
    for rev in (False, True):
        t = ", reverse" if rev else ""
        # a deletion in the A run (1000 ..) and one in the T run (1100 ..): 10 x 10 optima; both at their run's first base
        p.add("a deletion in each of two homopolymers" + t, 960, [("=", 45), ("D", 1), ("=", 99), ("D", 1), ("=", 40)], rev=rev, place=False, tie=True, route=DP1,
              want=lambda r: tied(r) and r["n_paths"] == 100 and r["cigar"] == [40 << 4, 1 << 4 | D, 99 << 4, 1 << 4 | D, 45 << 4] and r["md"] == "40^A99^T45")
        # an insertion of an A into the A run and a deletion in the T run: the band's two gap kinds tie in one record
        p.add("an insertion in one homopolymer, a deletion in another" + t, 960, [("=", 45), ("J", 1), ("=", 100), ("D", 1), ("=", 40)], rev=rev, place=False, tie=True, route=DP1,
              want=lambda r: tied(r) and r["cigar"] == [40 << 4, 1 << 4 | I, 100 << 4, 1 << 4 | D, 45 << 4] and r["md"] == "140^T45")
        # a repeat's deletion next to a forced insertion: five operations
        p.add("a deletion in a homopolymer and a forced insertion" + t, 960, [("=", 45), ("D", 1), ("=", 30), ("I", 2), ("=", 20)], rev=rev, place=False, tie=True, route=DP1,
              want=lambda r: tied(r) and r["n_paths"] == 10 and r["cigar"][:2] == [40 << 4, 1 << 4 | D] and r["n_cigar"] == 5)
        # the same in a band beyond 32: the wave kernel's backtrace answers in every mode
        p.add("a deletion in a homopolymer and an insertion of 30" + t, 960, [("=", 45), ("D", 1), ("=", 30), ("I", 30), ("=", 20)], rev=rev, place=False, tie=True, route=WAVE,
              want=lambda r: tied(r) and r["band"] > 32 and r["cigar"][:2] == [40 << 4, 1 << 4 | D] and r["n_cigar"] == 5)
        # two units of (AT) and the unit of (CAG) ... in one read they lie too far apart; a unit of (AT) deleted and an A of the A run far before it do not fit either:
        # (AT) alone with a forced deletion before it
        p.add("two units of (AT) deleted behind a forced deletion" + t, 2900, [("=", 30), ("D", 3), ("=", 73), ("D", 4), ("=", 40)], rev=rev, place=False, tie=True, route=DP1,
              want=lambda r: tied(r) and r["n_cigar"] == 5 and r["cigar"][2:4] == [67 << 4, 4 << 4 | D])
    parts.append(p)
    # -O 0: a gap of two costs what two gaps of one cost.  In a homopolymer the optima are many but the restated order still ends on ONE gap at the run's first
    # base; two windows found by search put the order itself on its seams:
    #   CACA against CCACAAC: 1D 3M 1D 1M 1D -- a gap that opens or extends at equal score opens (extending would give 1D 4M 2D);
    #   GAGCAA against AGAACA: at the LAST cell a diagonal step, a deletion and an insertion tie; the diagonal step is taken
    p = Part(wd, dict(o_del=0, o_ins=0))
    for rev in (False, True):
        t = ", reverse" if rev else ""
        p.add("-O 0, two bases of a homopolymer deleted" + t, 960, [("=", 45), ("D", 2), ("=", 45)], rev=rev, place=False, tie=True, w=3, route=DP0,
              want=lambda r: r["n_paths"] == 45 and r["leftmost"] == 40 and r["cigar"] == [40 << 4, 2 << 4 | D, 50 << 4] and r["md"] == "40^AA50")
        p.add_raw("-O 0, open or extend" + t, [1, 0, 1, 0], 3500, 7, rev=rev, truesc=1, tie=True, route=DP0,
                  want=lambda r: tied(r) and r["ties_met"]["oe"] >= 1 and r["band"] == 6 and r["cigar"] == [3 << 4, 1 << 4 | D, 1 << 4, 1 << 4 | D] and r["md"] == "3^A1" and r["pos"] == 3501 and r["raw_n_cigar"] == 5)
        p.add_raw("-O 0, three states tie at the last cell" + t, [2, 0, 2, 1, 0, 0], 3600, 6, rev=rev, truesc=0, tie=True, route=DP0,
                  want=lambda r: tied(r) and r["ties_met"]["h3"] >= 1 and r["band"] == 3 and r["n_paths"] == 7
                  and r["cigar"] == [2 << 4, 2 << 4 | I, 1 << 4, 1 << 4 | D, 1 << 4] and r["pos"] == 3601)
    parts.append(p)
    return Group("ties", "indels in homopolymers and tandem repeats on both strands: leftmost on the forward strand (ksw_global2 opens a gap from a diagonal step only, so a "
                 "mismatch never ties with an insertion next to a deletion); tied optima that are no single gap: the restated order", parts, ties=True)


def many_ops(wd, p, k, lead):
    """k gaps between k + 1 runs of 4 matches or a few more (so that no deletion can move), deletions and insertions in turn; with `lead' an insertion first"""
    s = [("I", 1)] if lead else []
    for i in range(k):
        n = 4
        while i % 2 == 0 and slides(wd, p, s + [("=", n), ("D", 1)]):
            n += 1
        s += [("=", n), ("D" if i % 2 == 0 else "I", 1)]
    return s + [("=", 4)]


def g_capacities():
    wd = world()
    parts = []
    O0 = dict(o_del=0, o_ins=0)
    for tag, opt, w in (("wave kernel", dict(O0), None), ("lane DP", dict(O0, w=2), 8)):
        p = Part(wd, opt)
        p.add("61 operations, " + tag, 80000, many_ops(wd, 80000, 30, False), w=w, place=False, want=lambda r: r["raw_n_cigar"] == 61, tie=False)
        p.add("62 operations, " + tag, 80400, many_ops(wd, 80400, 30, True), w=w, place=False, want=lambda r: r["raw_n_cigar"] == 62)
        parts.append(p)
        p = Part(wd, opt, overflow=6)
        p.add("63 operations, " + tag, 80800, many_ops(wd, 80800, 31, False), w=w, place=False, want=lambda r: r["raw_n_cigar"] == 63)
        parts.append(p)
    # an MD of 318 characters is the longest the record holds (319 and more: the call is refused): "100^" + 311 letters + "100" = 318
    for d, code in ((311, 0), (312, 7), (313, 7)):
        p = Part(wd, dict(w=400), overflow=code)
        p.add("a deletion of %d: an MD of %d characters" % (d, d + 7), 82000, [("=", 100), ("D", d), ("=", 100)], w=400, want=lambda r, d=d: r["l_md"] == d + 7 and r["band"] == d + 3)
        parts.append(p)
    # ... and from the gap-free kernel and the lane DP: 158 mismatches in a row are 316 characters, then the number of matches behind them.  -O 600 keeps the
    # DP from shifting the mismatching stretch; the lane DP gets the record through a truesc at the edge of the gap-free branch and a region's w of opt.w << 2
    for rest, code in ((42, 0), (100, 7)):
        p = Part(wd, dict(w=1, o_del=600, o_ins=600), overflow=code)
        p.add("158 mismatches and %d matches, gap-free" % rest, 84000, [("X", 158), ("=", rest)], want=lambda r, rest=rest: r["gap_free"] and r["l_md"] == 316 + len(str(rest)))
        p.add("158 mismatches and %d matches, lane DP" % rest, 84000, [("X", 158), ("=", rest)], truesc=158 + rest - 1200, w=4,
              want=lambda r, rest=rest: r["band"] == 3 and r["rounds"][0][0] == 4 and r["l_md"] == 316 + len(str(rest)))
        parts.append(p)
    # the direction matrix of the wave kernel: 192 columns x 1024 rows = 192 KiB exactly, x 1025 rows beyond
    for span, code in ((1024, 0), (1025, 5)):
        p = Part(wd, dict(w=1000), overflow=code)
        p.add("192 columns x %d rows" % span, 86000, [("=", 192), ("D", span - 192)], w=1000, want=lambda r, span=span: r["n_col_rows"] == 192 * span and (r["n_col_rows"] > rec.Z_CAP) == (span == 1025))
        parts.append(p)
    return Group("capacities", "62 / 63 operations, an MD of 318 / 319 / 320 characters, 192 KiB of direction cells and one row more: equal to the reference inside, SSG_EOVERFLOW beyond", parts)


def g_cell_range():
    wd = world()
    parts = []
    for o_ in (100, 1000, 3000, 5000, 7000, 8000, 9000, 12000, 16000, 30000):
        p = Part(wd, dict(o_del=o_, o_ins=o_), rule="cell_range")
        p.add("-O %d, a deletion of 4" % o_, 90000, [("=", 60), ("D", 4), ("=", 60)])
        p.add("-O %d, mismatches in band 3" % o_, 90300, mm(2, [10, 90], 120), truesc=120 - 2 * (o_ + 1 - 1))
        p.add("-O %d, an insertion of 2, reverse" % o_, 90600, [("=", 40), ("I", 2), ("=", 60)], rev=True)
        parts.append(p)
    for e_ in (40, 200, 400, 500):
        p = Part(wd, dict(e_del=e_, e_ins=e_), rule="cell_range")
        p.add("-E %d, a deletion of 20" % e_, 91000, [("=", 60), ("D", 20), ("=", 60)])
        parts.append(p)
    # the wave kernel's 32-bit cells at the limit the library states: open + 32769 x extend < 2^27
    p = Part(wd, dict(o_del=(1 << 27) - 32769 - 1, o_ins=(1 << 27) - 32769 - 1), rule="cell_range")
    p.add("gap open just inside the stated limit", 92000, [("=", 60), ("D", 4), ("=", 60)])
    parts.append(p)
    p = Part(wd, dict(e_del=4094, e_ins=4094, o_del=100, o_ins=100), rule="cell_range")
    p.add("gap extension just inside the stated limit", 92000, [("=", 60), ("D", 4), ("=", 60)])
    parts.append(p)
    return Group("cell_range", "gap penalties rising past the point where a reachable cell of the lane DP meets its minus infinity or leaves 16 bits; the wave kernel's at the stated limit", parts)


GROUPS = dict((f.__name__[2:], f) for f in (g_gap_free_edge, g_band_classes, g_ring_and_words, g_retry, g_wave_columns, g_end_gaps, g_strands_and_clips, g_contig_edges,
                                             g_query_n, g_ties, g_capacities, g_cell_range))
GROUP_NAMES = list(GROUPS)
_GROUPS = {}


def group(name):
    if name not in _GROUPS:
        _GROUPS[name] = GROUPS[name]()
    return _GROUPS[name]


# ------------------------------------------------------------------------------------------------------------------------------
# leg 1: the reference against itself
# ------------------------------------------------------------------------------------------------------------------------------
def test_infer_bw_and_w2_by_hand():
    # equal lengths: 0 below 2 (o + e - a) = 12; at it (100 - 88 - 6) / 1 + 2 = 8
    assert [rec.infer_bw(100, 100, s, 1, 6, 1) for s in (100, 90, 89, 88, 80)] == [0, 0, 0, 8, 16]
    # unequal lengths: never 0, at least the difference; the quotient is truncated toward zero ((95 - 100 - 6) / 2 + 2 = -3.5 -> -3 -> 5)
    assert rec.infer_bw(100, 95, 100, 1, 6, 2) == 5 and rec.infer_bw(95, 100, 60, 1, 6, 2) == 16 and rec.infer_bw(10, 12, -40, 1, 6, 4) == 13
    o = rec.opt_from()
    assert rec.w2_of(o, 100, 100, 50, 7) == 46 and rec.w2_of(o, 100, 100, -20, 7) == 7 and rec.w2_of(o, 100, 100, -20, 300) == 116
    assert rec.w2_of(rec.opt_from(o_ins=2), 100, 100, 88, 7) == 12                       # the larger of the two
    assert rec.w2_of(rec.opt_from(w=5), 100, 100, 88, 6) == 6 and rec.w2_of(rec.opt_from(w=5), 100, 100, 88, 20) == 8


def test_nm_md_and_the_text_they_rebuild():
    q = [0, 1, 2, 3, 0, 1, 2, 3, 0, 1]
    t = [0, 1, 2, 0, 0, 3, 3, 0, 2, 3, 0, 1]                       # three matches, a mismatch, a match, a deletion of TT, a mismatch, four matches
    cg = [(0, 5), (2, 2), (0, 5)]
    assert rec.nm_md(cg, q, t) == (4, "3A1^TT0A4")
    assert rec.rebuild(cg, "3A1^TT0A4", q) == t
    assert rec.nm_md([(2, 2), (0, 3), (1, 2), (0, 1), (2, 1)], [0, 1, 2, 3, 3, 0], [3, 3, 0, 1, 2, 0, 2]) == (2, "4")     # end deletions count nowhere; inserted bases in NM
    assert rec.nm_md([(0, 3)], [0, 4, 2], [0, 1, 2]) == (1, "1C1") and rec.nm_md([(0, 1)], [4], [0]) == (1, "0A0")
    assert rec.rebuild([(3, 2), (0, 3), (1, 1), (0, 2), (3, 1)], "1C3", [3, 3, 0, 0, 2, 1, 3, 0, 2], ) == [0, 1, 2, 3, 0]


def test_path_count_and_backtrace_on_small_cases():
    o = rec.opt_from()
    # AAAA against AAA: the deletion may lie at any of four places; the restated order puts it first
    m = rec.band_dp(o, [0, 0, 0], [0, 0, 0, 0], 3)
    assert m["n_paths"] == 4 and m["score"] == 3 - 7 and rec.backtrace(o, m, 4, 3) == [(2, 1), (0, 3)]
    # ACGT against AGT: forced
    m = rec.band_dp(o, [0, 2, 3], [0, 1, 2, 3], 3)
    assert m["n_paths"] == 1 and rec.backtrace(o, m, 4, 3) == [(0, 1), (2, 1), (0, 2)]
    # the band is a mask: a deletion of 4 does not fit a band of 3
    assert rec.band_dp(o, [0], [0, 1, 2, 3, 0], 3)["score"] <= rec.REACH and rec.band_dp(o, [0], [0, 1, 2, 3, 0], 4)["n_paths"] >= 1
    # the extremes of one cell
    m = rec.band_dp(o, [0], [0], 3)
    assert (m["lo"], m["hi"]) == (-7, 1)      # the boundary cells; the candidates 1 - 7 lie above them


def test_rounds_by_hand():
    o = rec.opt_from(w=5)
    q = [0, 1, 2, 3] * 10
    assert rec.rounds(o, q, q, 0, 40) == [(0, None, 40)]
    assert rec.rounds(o, q, q, 3, 40) == [(3, 3, 40)]                      # the score is there: one round
    assert rec.rounds(o, q, q, 3, 50) == [(3, 3, 40), (6, 6, 40)]           # it repeats
    assert rec.rounds(o, q, q, 20, 50) == [(20, 8, 40)]                     # opt.w << 2; the band itself is capped by what half the query pays for
    q2 = list(q); q2[7] = 0; q2[22] = 1
    assert rec.rounds(rec.opt_from(w=50), q2, q, 1, 50) == [(1, 3, 30), (2, 3, 30)]          # w2 doubles, the band is 3 both times, the score repeats


# ------------------------------------------------------------------------------------------------------------------------------
# leg 2: constructed groups
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GROUP_NAMES)
def test_group_reaches_its_boundary_on_the_reference(name):
    g = group(name)
    refs = group_reference(g)
    c = COUNTS[name]
    assert c["records"] >= 3
    if name == "ring_and_words":
        assert {0, 1, 7} <= g.widths(refs[0]), g.widths(refs[0])
    if name == "cell_range":
        o = [rec.opt_from(**p.opt) for p in g.parts]
        flags = [[beyond_lane_cells(r, oo) for r in rf if not r["gap_free"]] for rf, oo in zip(refs, o)]
        assert any(not any(f) for f in flags) and any(all(f) for f in flags), flags          # parts wholly inside and wholly beyond
        # the point itself: the first band's lowest reachable value is a gap candidate two openings deep, so it crosses -16384 + a between -O 5000 and -O 9000
        lo = {p.opt.get("o_del"): min(r["lo_first"] for r in rf) for p, rf in zip(g.parts, refs) if "e_del" not in p.opt}
        assert lo[5000] > R2D_NEG + 1 >= lo[9000], lo
    if name == "band_classes":
        assert set(c["bands"]) == {"3", "8", "9", "16", "17", "32", "33"} and all(v == 3 for v in c["bands"].values()), c["bands"]
    if name == "retry":
        assert set(c["rounds"]) == {"1", "2", "3"}
    if name == "ties":
        assert c["forced"] < c["records"]
        rest = [r for rf in refs for r in rf if r["n_paths"] > 1 and r["leftmost"] is None]
        assert sum(r["ties_met"]["oe"] for r in rest) >= 2 and sum(r["ties_met"]["h3"] for r in rest) >= 2 and sum(r["ties_met"]["h"] for r in rest) >= 20
        assert len(rest) >= 14 and any(r["is_rev"] for r in rest) and any(r["band"] > 32 for r in rest) and any(r["band"] <= 8 for r in rest), len(rest)
    elif name not in ("strands_and_clips",):
        assert c["forced"] == c["records"], c


@pytest.mark.parametrize("name", GROUP_NAMES)
def test_oracle_group_against_reference(name, oracle):
    check_group_oracle(group(name), oracle)


@pytest.mark.parametrize("name", GROUP_NAMES)
def test_emu_group_against_reference(name, emu_lib, monkeypatch):
    check_group_library(group(name), emu_lib, "the emulation build", monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GROUP_NAMES)
def test_gpu_group_against_reference(name, gpu_lib, monkeypatch):
    check_group_library(group(name), gpu_lib, "the HIP build", monkeypatch)


def refusal_cases(lib):
    """(what is wrong, keyword arguments that replace the valid call's, a word of the message)"""
    wd = world()
    part = Part(wd)
    part.add("v", 1000, [("=", 80), ("D", 2), ("=", 80)], lc=3, rc=4)
    part.add("v2", 3000, mm(1, [5], 60), rev=True)
    p = part.packed()
    L = wd.l_pac

    def ch(arr, f, v, k=0):
        b = arr.copy()
        if f is None:
            b[k] = v
        else:
            b[f][k] = v
        return b

    def opt_with(**kw):
        o = lib.opt_init()
        for k, v in kw.items():
            o[k] = v
        return o
    regs, req, off, seq = p["regs"], p["req"], p["off"], p["seq"]
    big = np.concatenate([seq[:off[1]], np.zeros(311 - off[1], np.uint8), seq[off[1]:]]).astype(np.uint8)
    cases = [("offsets that do not start at 0", dict(off=ch(off, None, 1)), "offsets"),
             ("offsets that decrease", dict(off=np.array([0, off[2], off[1]], np.int64)), "offsets"),
             ("an empty read", dict(off=np.array([0, 0, off[2]], np.int64)), "length"),
             ("a read of 311 bases", dict(seq=big, off=np.array([0, 311, 311 + off[2] - off[1]], np.int64)), "length"),
             ("a code of 5", dict(seq=ch(seq, None, 5, 17)), "codes"),
             ("qb < 0", dict(regs=ch(regs, "qb", -1)), "qb"),
             ("qb = qe", dict(regs=ch(regs, "qb", int(regs["qe"][0]))), "qb"),
             ("qe beyond the read", dict(regs=ch(regs, "qe", int(off[1]) + 1)), "qe"),
             ("rb < 0", dict(regs=ch(regs, "rb", -1)), "rb"),
             ("rb = re", dict(regs=ch(regs, "rb", int(regs["re"][0]))), "rb"),
             ("re beyond 2 l_pac", dict(regs=ch(ch(regs, "re", 2 * L + 1, 1), "rb", 2 * L - 50, 1)), "re"),
             ("a region across l_pac", dict(regs=ch(ch(regs, "rb", L - 40), "re", L + 42)), "boundary"),
             ("a window of 32769 bases", dict(regs=ch(regs, "re", int(regs["rb"][0]) + 32769)), "32768"),
             ("a read index of 2", dict(req=ch(req, "read", 2)), "read index"),
             ("a read index of -1", dict(req=ch(req, "read", -1)), "read index"),
             ("a region index of 2", dict(req=ch(req, "reg", 2)), "region index"),
             ("a kind of 2", dict(req=ch(req, "kind", 2)), "kind"),
             ("a region requested for a shorter read", dict(req=ch(req, "read", 1), regs=ch(regs, "qe", int(off[2] - off[1]) + 1)), "qe"),
             ("-w 65536", dict(opt=opt_with(w=65536)), "65535"), ("-w -1", dict(opt=opt_with(w=-1)), "65535"),
             ("-A 32", dict(opt=opt_with(a=32)), "score"), ("-B 33", dict(opt=opt_with(b=33)), "penalty"), ("-A 47", dict(opt=opt_with(a=47)), "score"),
             ("-A 25 with a read of 167 bases", dict(opt=opt_with(a=25)), "13-bit"),
             ("gap extension 0", dict(opt=opt_with(e_del=0)), "gap penalties"), ("gap open -1", dict(opt=opt_with(o_ins=-1)), "gap penalties"),
             ("gap open 2^27", dict(opt=opt_with(o_del=1 << 27)), "gap penalties"), ("gap extension 4096", dict(opt=opt_with(e_ins=4096)), "gap penalties"),
             ("contigs that do not tile", dict(ctg_len=[120000, 79999]), "tile"), ("l_pac = 0", dict(l_pac=0), "l_pac")]
    return wd, p, cases


def check_refusals(lib):
    wd, p, cases = refusal_cases(lib)

    def call(**kw):
        a = dict(p, opt=lib.opt_init(), l_pac=wd.l_pac, ctg_off=wd.ctg_off, ctg_len=wd.ctg_len)
        a.update(kw)
        return lib.dbg_reg2aln(a["opt"], wd.pac, a["l_pac"], a["ctg_off"], a["ctg_len"], a["seq"], a["off"], a["regs"], a["req"])
    rc, alns, route, err = call()
    assert (rc, err) == (0, 0) and list(route) == [DP0, LANE]
    for what, kw, word in cases:
        with pytest.raises(capi.SsgError) as e:
            call(**kw)
        assert "-22" in str(e.value) and word in str(e.value), (what, str(e.value))


def check_pipeline_refuses(lib):
    """gap penalties outside the CIGAR kernels' range end a pipeline call, and the region stage's entry, with SSG_EINVAL -- in run_align1, before the seeding stage"""
    import common
    _, seqs, seq, off = common.sim_reads(4, 7, 100, fasta=common.EXAMPLE_FA)
    idx = lib.index_load(common.EXAMPLE_FA)
    try:
        capi.mem_process_pairs(lib, idx, lib.opt_init(), seq, off, id0=0).close()
        for kw in (dict(e_del=0), dict(e_ins=0), dict(o_del=-1), dict(o_ins=1 << 27), dict(e_del=4096)):
            o = lib.opt_init()
            for k, v in kw.items():
                o[k] = v
            for call in (lambda: capi.mem_process_pairs(lib, idx, o, seq, off, id0=0), lambda: lib.align1_batch(idx, o, seq, off)):
                with pytest.raises(capi.SsgError) as e:
                    call()
                assert "-22" in str(e.value) and "gap penalties" in str(e.value), (kw, str(e.value))
    finally:
        lib.index_destroy(idx)


def test_emu_pipeline_refuses_gap_penalties(emu_lib):
    check_pipeline_refuses(emu_lib)


@pytest.mark.gpu
def test_gpu_pipeline_refuses_gap_penalties(gpu_lib):
    check_pipeline_refuses(gpu_lib)


def test_emu_refusals(emu_lib):
    check_refusals(emu_lib)


@pytest.mark.gpu
def test_gpu_refusals(gpu_lib):
    check_refusals(gpu_lib)


# ------------------------------------------------------------------------------------------------------------------------------
# leg 3: the regions and requests of simulated pairs, and the composition of the test entries
# ------------------------------------------------------------------------------------------------------------------------------
SSG_F_NO_RESCUE = 0x20
SIM_SETS = ((0.02, 0.01, 150), (0.05, 0.004, 150), (0.03, 0.01, 250), (0.01, 0.02, 101))     # (error, indel, length): test_emu_reg2aln_lane_dp_classes' settings
SIM_PAIRS = (50, 50, 30, 70)          # 200 pairs; fewer of the longest reads, whose reference is the slowest
_SIM, SIM_COUNTS = {}, {}


class IndexWorld:
    """the 2-bit reference and the contig table of an index on disk"""

    def __init__(self, prefix):
        ann = open(prefix + ".ann").read().split("\n")
        self.l_pac, n_seq = int(ann[0].split()[0]), int(ann[0].split()[1])
        pac = np.fromfile(prefix + ".pac", dtype=np.uint8)[:self.l_pac // 4 + 1]
        self.pac = np.concatenate([pac, np.zeros(self.l_pac // 4 + 1 - len(pac), np.uint8)])
        self.ctg_off = [int(ann[2 + 2 * i].split()[0]) for i in range(n_seq)]
        self.ctg_len = [int(ann[2 + 2 * i].split()[1]) for i in range(n_seq)]
        self.ref = rec.Ref(self.pac, self.l_pac, self.ctg_off, self.ctg_len)


def check_simulated(lib, oracle, k, who, monkeypatch):
    """without mate rescue the pairing stage's input is align1's lists: ssg_dbg_pair_final on them gives the regions and requests of ssg_mem_process_pairs, and
    ssg_dbg_reg2aln on those its records.  Reference == oracle == library, every request."""
    import common
    err, indel, rl = SIM_SETS[k]
    prefix = common.EXAMPLE_FA
    wd = IndexWorld(prefix)
    _, seqs, seq, off = common.sim_reads(SIM_PAIRS[k], 300 + k, rl, fasta=prefix, err=err, indel_frac=indel, ins_mean=500 if rl < 250 else 800, ins_std=60)
    idx = lib.index_load(prefix)
    opt = lib.opt_init()
    opt["flag"] |= SSG_F_NO_RESCUE
    res = capi.mem_process_pairs(lib, idx, opt, seq, off, id0=0)
    reg_off, regs, _ = lib.align1_batch(idx, opt, seq, off)
    regs_out, req_off, req = lib.dbg_pair_final(idx, opt, 0, reg_off, regs, res.pes[:4])
    lib.index_destroy(idx)
    assert np.array_equal(req_off, res.req_off) and len(req) == len(res.req)
    want = rows_of(res.alns)
    if k not in _SIM:            # the reference and the oracle, once
        o = rec.opt_from()
        refs = []
        for q in req:
            reg = None if q["reg"] < 0 else {f: int(regs_out[f][q["reg"]]) for f in ("rb", "re", "qb", "qe", "truesc", "w", "score", "sub", "csub", "secondary")}
            refs.append(rec.record(o, wd.ref, [int(c) for c in seqs[int(q["read"])]], reg, {f: int(q[f]) for f in ("kind", "owner", "flag", "mapq")}))
        oalns, over = oracle.reg2aln(wd.pac, wd.l_pac, wd.ctg_off, wd.ctg_len, seq, off, regs_out, req)
        assert not over.any()
        orows = rows_of(oalns)
        for i, (r, orow) in enumerate(zip(refs, orows)):
            assert row_of_ref(r) == orow, ("the oracle against the reference", SIM_SETS[k], i, row_of_ref(r), orow)
        dp_recs = [r for r in refs if "forced" in r and not r["gap_free"]]
        SIM_COUNTS["%g_%g_%d" % SIM_SETS[k]] = dict(pairs=SIM_PAIRS[k], records=len(refs), with_a_dp=len(dp_recs), forced=sum(r["forced"] for r in dp_recs),
                                                    forced_share_of_dp_records=round(sum(r["forced"] for r in dp_recs) / max(len(dp_recs), 1), 4),
                                                    tied_single_gap_in_a_repeat=sum(1 for r in dp_recs if not r["forced"] and r["leftmost"] is not None),
                                                    tied_restated_order_alone=sum(1 for r in dp_recs if not r["forced"] and r["leftmost"] is None),
                                                    ties_met_on_the_paths={k_: sum(r["ties_met"][k_] for r in dp_recs) for k_ in ("h", "h3", "oe")})
        _SIM[k] = (refs, [row_of_ref(r) for r in refs])
    refs, rrows = _SIM[k]
    assert want == rrows, (who, SIM_SETS[k], "the pipeline's records against the reference", next((a, b) for a, b in zip(want, rrows) if a != b))
    seen = set()
    for mode in ("1", "0"):
        monkeypatch.setenv("SSG_R2A_DPLANE", mode)
        rc, alns, route, e = lib.dbg_reg2aln(opt, wd.pac, wd.l_pac, wd.ctg_off, wd.ctg_len, seq, off, regs_out, req)
        assert (rc, e) == (0, 0)
        got = rows_of(alns)
        assert got == rrows, (who, SIM_SETS[k], mode, "ssg_dbg_pair_final -> ssg_dbg_reg2aln against the reference", next((a, b) for a, b in zip(got, rrows) if a != b))
        ml = max(len(x) for x in seqs)
        for q, r, rt in zip(req, refs, route):
            r["tlen"] = 0 if q["reg"] < 0 else int(regs_out["re"][q["reg"]] - regs_out["rb"][q["reg"]])
            assert int(rt) == expected_route(r, ml, mode == "1"), (who, SIM_SETS[k], mode, int(rt), r.get("rounds"))
            if mode == "1":
                seen.add(int(rt))
    monkeypatch.delenv("SSG_R2A_DPLANE", raising=False)
    res.close()
    return seen


_EMU_SEEN = {}


@pytest.mark.parametrize("k", range(len(SIM_SETS)))
def test_emu_simulated_reads_against_reference(k, emu_lib, oracle, monkeypatch):
    _EMU_SEEN[k] = check_simulated(emu_lib, oracle, k, "the emulation build", monkeypatch)
    SIM_COUNTS.setdefault("routes_emulation", set()).update(_EMU_SEEN[k])


def test_emu_simulated_reads_fill_every_route(emu_lib, oracle, monkeypatch):
    """the gap-free lane kernel, all three classes of the lane DP and the wave kernel each have records among the four sets (those that have not run yet run here)"""
    for k in range(len(SIM_SETS)):
        if k not in _EMU_SEEN:
            _EMU_SEEN[k] = check_simulated(emu_lib, oracle, k, "the emulation build", monkeypatch)
    seen = set().union(*_EMU_SEEN.values())
    assert all(any(rt & c for rt in seen) for c in (LANE, DP0, DP1, DP2, WAVE)), seen


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(SIM_SETS)))
def test_gpu_simulated_reads_against_reference(k, gpu_lib, oracle, monkeypatch):
    check_simulated(gpu_lib, oracle, k, "the HIP build", monkeypatch)


def test_zz_what_the_reference_evaluated():
    """Over every constructed group -- evaluated here unless a test above has done so: records, forced CIGARs, rounds, final bands, routes.  Where
    SSG_RECORD_COUNTS_OUT names a directory the figures go to record_reference_groups.json there, and those of the simulated sets that ran (the share of
    records whose CIGAR was forced, per setting: a recorded fact, not a threshold) to record_reference_simulated.json."""
    for n in GROUP_NAMES:
        group_reference(group(n))
    assert sum(COUNTS[n]["records"] for n in GROUP_NAMES) >= 200
    routes = set(int(k) for n in GROUP_NAMES for k in COUNTS[n]["routes"])
    assert {0, LANE, DP0, DP1, DP2, WAVE, DP0 | WAVE, DP1 | WAVE} <= routes, routes
    out = os.environ.get("SSG_RECORD_COUNTS_OUT")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "record_reference_groups.json"), "w") as f:
            json.dump(COUNTS, f, indent=1, sort_keys=True)
        with open(os.path.join(out, "record_reference_simulated.json"), "w") as f:
            json.dump({k: (sorted(v) if isinstance(v, set) else v) for k, v in SIM_COUNTS.items()}, f, indent=1, sort_keys=True)
