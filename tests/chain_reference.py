"""Independent reference of the chaining stage (upstream mem_chain with test_and_merge, mem_chain_weight, mem_chain_flt and the frac_rep of mem_chain's
head) -- TEST INFRASTRUCTURE ONLY.

Written from SURVEY.md Appendix B and upstream's documented behaviour (bwamem.c), not from csrc/k_chain.h, csrc/k_chainw.h or oracle/orc_mem.c.  It
imports neither oracle_py nor speedseq_amd.capi, and shares with them the option names and nothing else: no tree, no linked list, no packed word, no
numpy on a decision path (numpy appears in the self-tests of tests/test_chain_reference.py only).  Integers, fractions.Fraction, lists and sets.

What is a DEFINITION here (stated as a set or a closed expression, no loop that stops early, no container):
  * frac_rep    the measure of a union of query intervals, as a set of positions, over the read length, rounded once to binary32;
  * weight      per axis, the number of positions of seed j at or beyond every earlier seed's end; the smaller of the two axes, capped;
  * f32         round-to-nearest-even of an exact Fraction to binary32;
  * the candidate of a seed in `chains': the chain of greatest position <= rbeg, found by looking at every chain.
What is a SECOND RESTATEMENT (the operation has no statement as a set: it is greedy and order dependent, so it is the loop again, in another hand, as
dp_reference.py says of the extension and pair_reference.py of mem_mark_primary_se):
  * `chains'    the greedy insertion in visiting order with test_and_merge as four named predicates;
  * `flt'       mem_chain_flt's scan against the kept list with its side effects (large_ovlp, first, kept 1 / 2 / 3) and the max_chain_extend cut.

Where the answer is not decided here.  Upstream keeps a read's chains in klib's B-tree keyed by position with equal keys allowed; which of several chains
at ONE position a look-up meets, and where a new one lands among them, is a property of that container, which is [RECALL] (kbtree.h is not in the reference
tree) and has no independent statement.  `chains' reports such reads (shared_position) and the tests leave them to the oracle.  The order mem_chain_flt's
unstable sort leaves among EQUAL weights is the other: a read whose weights are all distinct is ordered here; otherwise the caller passes the order the
oracle's ks_introsort restatement left (pinned to reference-held bytes elsewhere), and `flt' checks that it is a permutation of its own chains with
non-increasing weights before it uses it.

The two float comparisons of the filter -- e_min - b_max >= min_l * mask_level and w_i < w_j * drop_ratio -- are evaluated twice: exactly, with the option's
binary32 value as a Fraction, and as C does it, with the product rounded once to binary32 (the integer sides are below 2^24 and convert exactly).  The C
form decides; a site where the two disagree is a NEAR site and is recorded in the Tally.
"""
from fractions import Fraction as F

DEFAULTS = dict(w=100, max_chain_gap=10000, min_seed_len=19, max_occ=500, mask_level=0.5, drop_ratio=0.5, min_chain_weight=0, max_chain_extend=1 << 30)
W_CAP = (1 << 30) - 1


def f32(x):
    """the binary32 nearest to the exact rational x (ties to even), as a Fraction; normal and subnormal range, no overflow handling beyond an assertion"""
    x = F(x)
    if x == 0:
        return F(0)
    s, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()   # 2^(e-1) < a < 2^(e+1)
    if F(2) ** e > a:
        e -= 1                                                  # now 2^e <= a < 2^(e+1)
    assert e < 128, "beyond binary32"
    q = max(e, -126) - 23                                       # the unit in the last place: 24 significant bits, or the subnormal grid
    t = a / F(2) ** q
    n, r = divmod(t.numerator, t.denominator)
    twice = 2 * r
    if twice > t.denominator or (twice == t.denominator and n & 1):
        n += 1
    return s * n * F(2) ** q


def f32_bits(x):
    """the IEEE-754 binary32 bit pattern of f32(x), for bit-for-bit comparison with a stored float"""
    v = f32(x)
    if v == 0:
        return 0
    s, a = (1 << 31 if v < 0 else 0), abs(v)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if F(2) ** e > a:
        e -= 1
    if e < -126:
        return s | int(a / F(2) ** -149)
    m = int(a / F(2) ** (e - 23))
    return s | (e + 127) << 23 | (m - (1 << 23))


def opt_from(rec=None, **kw):
    """the option values this stage reads, from a record with those field names or the defaults, then kw; the two floats enter at their binary32 values"""
    o = dict(DEFAULTS)
    if rec is not None:
        for k in DEFAULTS:
            o[k] = rec[k].item() if hasattr(rec[k], "item") else rec[k]
    o.update(kw)
    for k in ("mask_level", "drop_ratio"):
        o[k] = f32(F(o[k]))
    return o


class Tally:
    """the float comparison sites of an evaluation: how many, and which were near (exact and binary32 answers differ)"""

    def __init__(self):
        self.n = 0
        self.near = []
        self._products = {}

    def add(self, other):
        self.n += other.n
        self.near += other.near

    def _product(self, n, c):
        """(n * c exactly, n * c rounded once to binary32), remembered per (n, c)"""
        if (n, c) not in self._products:
            self._products[(n, c)] = (n * c, f32(n * c))
        return self._products[(n, c)]

    def _site(self, what, exact, as_c):
        self.n += 1
        if exact != as_c:
            self.near.append(what)
        return as_c

    def ge_prod(self, lhs, n, c, what):
        """lhs >= n * c as C evaluates it for int lhs, int n, float c"""
        exact, rounded = self._product(n, c)
        return self._site((what, lhs, n, c), lhs >= exact, lhs >= rounded)

    def lt_prod(self, lhs, n, c, what):
        """lhs < n * c, likewise"""
        exact, rounded = self._product(n, c)
        return self._site((what, lhs, n, c), lhs < exact, lhs < rounded)


# ---------------------------------------------------------------- frac_rep
def frac_rep(opt, read_len, intervals):
    """intervals: (start, end, occurrences) in the order of the read's interval list, which upstream sorts by start.  Returns (l_rep, binary32 bits of
    l_rep / read_len)."""
    starts = [s for s, _, _ in intervals]
    if any(starts[i] > starts[i + 1] for i in range(len(starts) - 1)):
        raise ValueError("frac_rep: intervals not sorted by start -- upstream's running merge equals the union only for sorted input")
    covered = set()
    for s, e, occ in intervals:
        if occ > opt["max_occ"]:
            covered.update(range(s, e))
    l_rep = len(covered)
    return l_rep, f32_bits(F(l_rep, read_len))


# ---------------------------------------------------------------- mem_chain
def same_contig(chain_rid, rid):
    return chain_rid == rid


def contained(first, last, s):
    """inside the rectangle from the chain's first seed's begins to its last seed's ends, on both axes"""
    return s[1] >= first[1] and s[1] + s[2] <= last[1] + last[2] and s[0] >= first[0] and s[0] + s[2] <= last[0] + last[2]


def crosses_strand(l_pac, first, last, s):
    """a chain with an end on the forward strand never takes a seed on the reverse strand"""
    return (last[0] < l_pac or first[0] < l_pac) and s[0] >= l_pac


def colinear(opt, last, s):
    x, y = s[1] - last[1], s[0] - last[0]
    return y >= 0 and abs(x - y) <= opt["w"] and x - last[2] < opt["max_chain_gap"] and y - last[2] < opt["max_chain_gap"]


def test_and_merge(opt, l_pac, chain, seeds, i):
    """(accepted, appended) for seed i against the chain [pos, rid, [seed indices]]"""
    s, first, last = seeds[i], seeds[chain[2][0]], seeds[chain[2][-1]]
    if not same_contig(chain[1], s[3]):
        return False, False
    if contained(first, last, s):
        return True, False
    if crosses_strand(l_pac, first, last, s):
        return False, False
    if colinear(opt, last, s):
        return True, True
    return False, False


def chains(opt, l_pac, seeds):
    """seeds: (rbeg, qbeg, len, rid) in visiting order.  Returns (chains as (pos, rid, [seed indices]) by ascending position -- creation order among equal
    positions, which is NOT a claim about upstream's order there --, shared_position, info).  info: which branches were taken, for the tests' conditions."""
    made, positions = [], []          # chains in creation order, and their positions beside them
    shared = False
    info = dict(contained=0, appended=0, refused_contig=0, refused_strand=0, refused_band=0, below_all=0, new=0, skipped=0)
    for i, s in enumerate(seeds):
        if s[3] < 0:
            info["skipped"] += 1
            continue
        floor_pos = max((p for p in positions if p <= s[0]), default=None)     # every chain is looked at: no search structure
        cand = None
        if floor_pos is not None:
            if positions.count(floor_pos) > 1:
                shared = True
            cand = made[positions.index(floor_pos)]
        elif made:
            info["below_all"] += 1
        ok = False
        if cand is not None:
            ok, app = test_and_merge(opt, l_pac, cand, seeds, i)
            if ok and app:
                cand[2].append(i)
                info["appended"] += 1
            elif ok:
                info["contained"] += 1
            else:
                first, last = seeds[cand[2][0]], seeds[cand[2][-1]]
                if not same_contig(cand[1], s[3]):
                    info["refused_contig"] += 1
                elif crosses_strand(l_pac, first, last, s):
                    info["refused_strand"] += 1
                else:
                    info["refused_band"] += 1
        if not ok:
            if s[0] in positions:
                shared = True
            made.append([s[0], s[3], [i]])
            positions.append(s[0])
            info["new"] += 1
    order = sorted(range(len(made)), key=lambda k: (made[k][0], k))
    return [(made[k][0], made[k][1], list(made[k][2])) for k in order], shared, info


def chains_brute(opt, l_pac, seeds):
    """`chains' with the candidate found another way (self-test): scan positions downwards from rbeg over a dict of position -> chains"""
    by_pos, made = {}, []
    for i, s in enumerate(seeds):
        if s[3] < 0:
            continue
        cand = None
        for p in sorted(by_pos, reverse=True):
            if p <= s[0]:
                cand = by_pos[p][0]
                break
        ok = False
        if cand is not None:
            ok, app = test_and_merge(opt, l_pac, cand, seeds, i)
            if ok and app:
                cand[2].append(i)
        if not ok:
            c = [s[0], s[3], [i]]
            by_pos.setdefault(s[0], []).append(c)
            made.append(c)
    return sorted(((c[0], c[1], list(c[2])) for c in made), key=lambda c: (c[0], c[2][0]))


# ---------------------------------------------------------------- mem_chain_weight
def _axis_weight(spans):
    """spans: (begin, length) in the chain's order: positions of span j at or beyond max(0, every earlier end)"""
    w, reach = 0, 0
    for b, l in spans:
        w += max(0, b + l - max(b, reach))
        reach = max(reach, b + l)
    return w


def weight(seeds_of_chain):
    """seeds_of_chain: the chain's (rbeg, qbeg, len, ...) in insertion order"""
    wq = _axis_weight([(s[1], s[2]) for s in seeds_of_chain])
    wr = _axis_weight([(s[0], s[2]) for s in seeds_of_chain])
    return min(wq, wr, W_CAP)


def weight_sets(seeds_of_chain):
    """the same from explicit position sets (self-test), and the measure of the union on each axis"""
    out, unions = [], []
    for ax in (1, 0):
        w, reach, union = 0, 0, set()
        for s in seeds_of_chain:
            w += len([p for p in range(s[ax], s[ax] + s[2]) if p >= reach])
            reach = max(reach, s[ax] + s[2])
            union.update(range(s[ax], s[ax] + s[2]))
        out.append(w)
        unions.append(len(union))
    return min(out[0], out[1], W_CAP), out, unions


# ---------------------------------------------------------------- mem_chain_flt
def tie_free(opt, weights):
    w = [x for x in weights if x >= opt["min_chain_weight"]]
    return len(set(w)) == len(w)


def flt(opt, seeds, chain_list, weights, order=None, tally=None):
    """chain_list: (pos, rid, [seed indices]); weights: one per chain.  Returns the chains that pass min_chain_weight in sorted order, those the filter
    drops included, as (index into chain_list, kept); the survivors are those with kept != 0, in that order.  order: indices into chain_list in the order
    the sort left them, needed when weights tie."""
    tally = tally if tally is not None else Tally()
    cand = [k for k in range(len(chain_list)) if weights[k] >= opt["min_chain_weight"]]
    if not cand:
        return []
    if order is None:
        if not tie_free(opt, weights):
            raise ValueError("flt: weights tie and no order was given")
        order = sorted(cand, key=lambda k: -weights[k])
    else:
        order = list(order)
        if sorted(order) != cand:
            raise ValueError("flt: the given order is not a permutation of the chains that pass min_chain_weight")
        if any(weights[order[k]] < weights[order[k + 1]] for k in range(len(order) - 1)):
            raise ValueError("flt: the given order is not by non-increasing weight")
    beg = [seeds[c[2][0]][1] for c in chain_list]                        # a chain's query span: its first seed's begin to its LAST seed's end
    end = [seeds[c[2][-1]][1] + seeds[c[2][-1]][2] for c in chain_list]
    kept, first, kept_list = {order[0]: 3}, {}, [order[0]]
    for i in order[1:]:
        large_ovlp, dropped = False, False
        bi, ei = beg[i], end[i]
        for j in [k for k in kept_list if end[k] > bi and beg[k] < ei]:     # (the kept chains that can overlap this one at all, in their order: the others have no effect)
            bj, ej = beg[j], end[j]
            b_max, e_min = (bj if bj > bi else bi), (ej if ej < ei else ei)
            if e_min <= b_max:
                continue
            min_l = min(ei - bi, ej - bj)
            if tally.ge_prod(e_min - b_max, min_l, opt["mask_level"], "mask_level") and min_l < opt["max_chain_gap"]:
                large_ovlp = True
                first.setdefault(j, i)
                if tally.lt_prod(weights[i], weights[j], opt["drop_ratio"], "drop_ratio") and weights[j] - weights[i] >= 2 * opt["min_seed_len"]:
                    dropped = True
                    break
        if dropped:
            kept[i] = 0
        else:
            kept_list.append(i)
            kept[i] = 2 if large_ovlp else 3
    for j in kept_list:
        if j in first:
            kept[first[j]] = 1
    cut, n_ext = len(order), 0
    for at, i in enumerate(order):
        if kept[i] in (0, 3):
            continue
        n_ext += 1
        if n_ext >= opt["max_chain_extend"]:
            cut = at
            break
    for i in order[cut:]:
        if kept[i] < 3:
            kept[i] = 0
    return [(i, kept[i]) for i in order]


def read(opt, l_pac, read_len, seeds, intervals, order_of=None, tally=None):
    """one read through the whole stage.  order_of: None, or a function (chain_list, weights) -> order for reads whose weights tie.  Returns a dict:
    chains, shared_position, info, weights, tie_free, marks (flt's list), survivors as (pos, rid, seed tuple, w, kept), l_rep, frac_rep_bits."""
    cl, shared, info = chains(opt, l_pac, seeds)
    ws = [weight([seeds[i] for i in c[2]]) for c in cl]
    tf = tie_free(opt, ws)
    order = None if tf or shared or order_of is None else order_of(cl, ws)
    marks = flt(opt, seeds, cl, ws, order, tally) if not shared and (tf or order is not None) else None     # a read with a shared position is reported, not decided
    l_rep, fbits = frac_rep(opt, read_len, intervals)
    out = dict(chains=cl, shared_position=shared, info=info, weights=ws, tie_free=tf, marks=marks, l_rep=l_rep, frac_rep_bits=fbits)
    if marks is not None:
        out["survivors"] = [(cl[i][0], cl[i][1], tuple(cl[i][2]), ws[i], k) for i, k in marks if k]
    return out
