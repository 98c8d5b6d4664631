"""Mate rescue's list logic on compact keys (csrc/k_mswkeys.h: ssg_k_matesw_keys, with ssg_k_matesw for what that kernel leaves) against
tests/matesw_reference.py -- upstream mem_matesw and mem_sort_dedup_patch restated, window alignments from the oracle's orc_api_align2 -- through
ssg_dbg_matesw, the pipeline's own host code on region lists given here.

Inputs.  Reads are cut from the index's own text, so every alignment is known: an anchor region of one read at P and the mate's piece an insert
size further on, just OUTSIDE the insert-size window the model allows (dist < low), so that mem_matesw's skip test does not see the regions placed
next to the rescued hit.  Lists are lengthened with decoy regions far away on the other strand, sorted by (score, rb) and never redundant with one
another: a fixed point of mem_sort_dedup_patch (fixed = 1: the incremental re-sort) that is also given as `not yet re-sorted' (fixed = 0: the full
sort).  Tie-free inputs go through the reference, which raises on any tie; the inputs with ties, and the pairs the key kernel cannot decide, are
compared with the SSG_MSW_KEYS=0 run.
Each case runs on the emulator and, marked gpu, on the device.
"""
import numpy as np
import pytest

import common
import matesw_reference as MR
from speedseq_amd import capi

PREFIX = common.EXAMPLE_FA
SSG_SDP_CAP, SSG_SDP_BIG, SSG_ML_TMAX = 256, 2048, 8192
INS, LOW, HIGH = 400, 410, 800          # the mate ends INS after the anchor's start; the model allows [LOW, HIGH]
RL = 150
_WORLD = {}


def world(lib, oracle):
    if "ref" not in _WORLD:
        _WORLD["ref"] = MR.Ref(PREFIX)
    key = id(lib)
    if key not in _WORLD:
        _WORLD[key] = lib.index_load(PREFIX)
    return _WORLD["ref"], _WORLD[key]


def pes_array(models):
    pes = np.zeros(4, dtype=capi.PESTAT_DT)
    pes["failed"] = 1
    for r, (lo, hi) in models.items():
        pes[r] = (lo, hi, 0, 0, (lo + hi) / 2.0, 50.0)
    return pes


def region(rb, re, qb, qe, score, **kw):
    d = MR.new_region()
    d.update(rb=rb, re=re, qb=qb, qe=qe, score=score, rid=0, secondary=-1, seedcov=min(re - rb, qe - qb) >> 1, n_comp=0)
    d.update(kw)
    return d


def to_array(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    arr = np.zeros(int(off[-1]), dtype=capi.ALNREG_DT)
    k = 0
    for x in lists:
        for d in x:
            for f in MR.FIELDS:
                arr[k][f] = d[f]
            k += 1
    return off, arr


def revcomp(x):
    return (3 - x[::-1]).astype(np.uint8)


class Pair:
    """read 1 = the pieces t2[P : P + K] of its anchors one after another, read 2 = the reverse complement of the mates' pieces t2[P + INS - L : P + INS];
    `a' pieces have their region in read 1's list (they rescue into read 2's), `d' pieces have their mate's region in read 2's list (they rescue
    into read 1's); the rest of a read is random"""

    def __init__(self, R, seed, a=(), d=(), fixed=(1, 1)):
        rng = np.random.default_rng(seed)
        r1, f2 = rng.integers(0, 4, RL).astype(np.uint8), rng.integers(0, 4, RL).astype(np.uint8)
        self.lists = [[], []]
        o1 = o2 = 0
        for P, K, L in a:
            r1[o1:o1 + K] = R.t2[P:P + K]
            f2[o2:o2 + L] = R.t2[P + INS - L:P + INS]
            self.lists[0].append(region(P, P + K, o1, o1 + K, K))
            o1, o2 = o1 + K, o2 + L
        for P, K, L in d:
            r1[o1:o1 + K] = R.t2[P:P + K]
            f2[o2:o2 + L] = R.t2[P + INS - L:P + INS]
            self.lists[1].append(region(2 * R.l_pac - (P + INS), 2 * R.l_pac - (P + INS) + L, RL - (o2 + L), RL - o2, L))
            o1, o2 = o1 + K, o2 + L
        assert o1 <= RL and o2 <= RL
        self.reads = (r1, revcomp(f2))
        self.fixed = list(fixed)
        for t in range(2):
            self.lists[t].sort(key=lambda r: (-r["score"], r["rb"], r["qb"]))

    def add_decoys(self, t, n, first=60, rest=None):
        """fills read t's list up to n regions with regions far from every window, on the forward strand: 100 bases every 50; the first scores `first', the
        others at least 18 less, falling with the position -- so only the first can be an anchor (a hit within pen_unpaired of the best)"""
        have = len(self.lists[t])
        rest = first - 18 if rest is None else rest
        for k in range(n - have):
            rb = 200000 + 50 * k
            self.lists[t].append(region(rb, rb + 100, 0, 100, first if k == 0 else max(1, rest - k // 128)))
        self.lists[t].sort(key=lambda r: (-r["score"], r["rb"], r["qb"]))
        assert len(self.lists[t]) == n


def sealed(p):
    """the pair's lists as they are handed over: a list called a fixed point is the output of mem_sort_dedup_patch, which leaves n_comp = 1 in every
    region of a list of two or more"""
    out = []
    for t in range(2):
        out.append([dict(r, n_comp=1) if p.fixed[t] and len(p.lists[t]) > 1 else dict(r) for r in p.lists[t]])
    return out


def run_lib(lib, idx, pairs, pes, headroom=-1):
    seq = np.concatenate([r for p in pairs for r in p.reads])
    roff = np.arange(2 * len(pairs) + 1, dtype=np.int64) * RL
    off, arr = to_array([l for p in pairs for l in sealed(p)])
    fixed = np.array([f for p in pairs for f in p.fixed], dtype=np.uint8)
    return lib.dbg_matesw(idx, lib.opt_init(), seq, roff, off, arr, pes, fixed=fixed, headroom=headroom)


def reference(oracle, R, lib, pairs, pes):
    opt = MR.opt_from(lib.opt_init()[0])
    rp = [dict(low=int(p["low"]), high=int(p["high"]), failed=int(p["failed"])) for p in pes]
    out, windows = [], 0
    for p in pairs:
        a, tally = MR.rescue_pair(opt, R, rp, p.reads, sealed(p), lambda q, t, x: oracle.align2(q, t, x))   # raises MR.Tie: the input is not tie-free
        out += a
        windows += tally["windows"]
    return out, windows


def same_lists(got, want, who):
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), "%s: read %d has %d regions, the reference %d" % (who, r, len(g), len(w))
        for k, d in enumerate(w):
            for f in MR.FIELDS:
                assert g[k][f] == d[f], "%s: read %d region %d field %s: %r, the reference %r" % (who, r, k, f, g[k][f], d[f])


def same_as_old(lib, idx, pairs, pes, monkeypatch, headroom=-1):
    """the run with the key kernel and the SSG_MSW_KEYS=0 run: lists, error codes and counters"""
    monkeypatch.setenv("SSG_MSW_KEYS", "0")
    l0, e0, c0 = run_lib(lib, idx, pairs, pes, headroom)
    monkeypatch.delenv("SSG_MSW_KEYS")
    l1, e1, c1 = run_lib(lib, idx, pairs, pes, headroom)
    assert int(c0[2]) == 0 and int(c0[3]) == int(c0[4])
    assert np.array_equal(e0, e1), (e0, e1)
    assert [int(c1[k]) for k in (0, 1, 4, 5)] == [int(c0[k]) for k in (0, 1, 4, 5)], (c0, c1)
    assert len(l0) == len(l1)
    for r, (x, y) in enumerate(zip(l0, l1)):
        assert x.tobytes() == y.tobytes(), "read %d differs from the SSG_MSW_KEYS=0 run" % r
    return l1, e1, c1


def check_tie_free(lib, oracle, pairs, pes, monkeypatch, all_taken=True):
    R, idx = world(lib, oracle)
    want, windows = reference(oracle, R, lib, pairs, pes)
    for keys in ("1", "0"):
        monkeypatch.setenv("SSG_MSW_KEYS", keys)
        got, err, cnt = run_lib(lib, idx, pairs, pes)
        same_lists(got, want, "SSG_MSW_KEYS=" + keys)
        assert not err.any() and int(cnt[0]) == windows
        if keys == "1" and all_taken:
            assert int(cnt[3]) == 0 and int(cnt[2]) == int(cnt[4]) == len(pairs) and int(cnt[1]) == windows, cnt
    monkeypatch.delenv("SSG_MSW_KEYS", raising=False)
    return want


FR = {1: (LOW, HIGH)}
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, SSG_SDP_BIG)


def length_pairs(R, fixed):
    """one anchor of read 1, two pieces of the mate rescued into a list of the given length (the second hit crosses SSG_SDP_CAP where the first does not)"""
    out = []
    for k, n in enumerate(LENGTHS):
        p = Pair(R, 100 + k, a=[(20000 + 7000 * k, 70, 60), (24000 + 7000 * k, 70, 65)], fixed=(1, fixed))
        p.add_decoys(1, n)
        out.append(p)
    return out


def case_lengths(lib, oracle, monkeypatch, fixed):
    R, _ = world(lib, oracle)
    pairs = length_pairs(R, fixed)
    want = check_tie_free(lib, oracle, pairs, pes_array(FR), monkeypatch)
    for k, n in enumerate(LENGTHS):
        assert len(want[2 * k + 1]) == n + 2, "both hits of the mate are rescued and stay"


def case_too_long(lib, oracle, monkeypatch):
    """a list of SSG_SDP_BIG + 1 entries is left to ssg_k_matesw"""
    R, idx = world(lib, oracle)
    p = Pair(R, 140, a=[(30000, 70, 60)])
    p.add_decoys(1, SSG_SDP_BIG + 1)
    pes = pes_array(FR)
    want = check_tie_free(lib, oracle, [p], pes, monkeypatch, all_taken=False)
    assert len(want[1]) == SSG_SDP_BIG + 2
    _, _, cnt = same_as_old(lib, idx, [p], pes, monkeypatch)
    assert int(cnt[2]) == 0 and int(cnt[3]) == 1


def case_both_sides(lib, oracle, monkeypatch):
    """three anchors a side, both sides rescuing: a list carries over from window to window, the second side's anchors are the first side's list as it was"""
    R, _ = world(lib, oracle)
    pairs = []
    for fixed in ((1, 1), (0, 0)):
        p = Pair(R, 150, a=[(40000, 25, 25), (47000, 25, 25), (54000, 25, 25)], d=[(61000, 25, 25), (68000, 25, 25), (75000, 25, 25)], fixed=fixed)
        p.add_decoys(0, 40, first=20)
        p.add_decoys(1, 70, first=20)
        pairs.append(p)
    want = check_tie_free(lib, oracle, pairs, pes_array(FR), monkeypatch)
    assert len(want[0]) == 43 and len(want[1]) == 73


def rescued_hit(lib, oracle, p, pes):
    R, _ = world(lib, oracle)
    want, _ = reference(oracle, R, lib, [p], pes)
    assert len(want[1]) == len(p.lists[1]) + 1
    return [r for r in want[1] if not any(r["rb"] == y["rb"] and r["re"] == y["re"] for y in p.lists[1])][0]


def drop_pair(R, seed=160):
    return Pair(R, seed, a=[(90000, 140, 120)])


def case_drops(lib, oracle, monkeypatch):
    """regions next to the rescued hit x: an earlier-ending better one drops x; a later-ending one drops x; x drops several worse ones on both sides.
    The neighbours are short regions inside x: redundant with x, not with one another (a fixed point)."""
    R, _ = world(lib, oracle)
    pes = pes_array(FR)
    x = rescued_hit(lib, oracle, drop_pair(R), pes)
    assert x["re"] - x["rb"] >= 120 and x["score"] >= 120

    def inside(at, score, n=20):   # [at, at + n) of x's reference and query intervals
        return region(x["rb"] + at, x["rb"] + at + n, x["qb"] + at, x["qb"] + at + n, score)

    def over_end(score):           # 26 bases that end one past x on the reference
        return region(x["re"] - 25, x["re"] + 1, x["qe"] - 26, x["qe"], score)

    cases = dict(earlier_better=([inside(30, 500)], 1), later_better=([over_end(500)], 1), later_equal=([over_end(x["score"])], 1),
                 x_drops_many=([inside(10, 30), inside(40, 31), inside(70, 32), over_end(33)], 1))
    pairs, names = [], []
    for name, (extra, keep) in cases.items():
        for fixed in (1, 0):
            p = drop_pair(R)
            p.fixed = [1, fixed]
            p.lists[1] = sorted(extra, key=lambda r: (-r["score"], r["rb"], r["qb"]))
            p.add_decoys(1, len(extra) + 30, first=600, rest=10)
            pairs.append(p)
            names.append(name)
    want = check_tie_free(lib, oracle, pairs, pes, monkeypatch)
    for k, name in enumerate(names):
        got = want[2 * k + 1]
        has_x = any(r["rb"] == x["rb"] and r["re"] == x["re"] for r in got)
        if name == "x_drops_many":
            assert has_x and len(got) == 31, name
        else:
            assert not has_x and len(got) == 31, name


def case_leftover(lib, oracle, monkeypatch):
    """a window longer than SSG_ML_TMAX has no slot; a slice without head-room cannot take the hit: both pairs are left to ssg_k_matesw, and lists, error
    codes and counters are those of the SSG_MSW_KEYS=0 run"""
    R, idx = world(lib, oracle)
    wide = pes_array({1: (LOW, LOW + SSG_ML_TMAX + 500)})
    p = Pair(R, 170, a=[(100000, 70, 60)])
    p.add_decoys(1, 5)
    want = check_tie_free(lib, oracle, [p], wide, monkeypatch, all_taken=False)
    assert len(want[1]) == 6
    _, err, cnt = same_as_old(lib, idx, [p], wide, monkeypatch)
    assert int(cnt[3]) == 1 and int(cnt[2]) == 0 and int(cnt[1]) < int(cnt[0]) and not err.any()
    q = Pair(R, 171, a=[(110000, 70, 60)])
    q.add_decoys(1, 5)
    lists, err, cnt = same_as_old(lib, idx, [q], pes_array(FR), monkeypatch, headroom=0)
    assert int(cnt[3]) == 1 and int(cnt[2]) == 0 and int(err[0]) == 2 and len(lists[1]) == 5


def case_ties(lib, oracle, monkeypatch):
    """the rescued hit equals an old region on `re', and on (score, rb, qb): upstream's unstable sorts decide, so the reference refuses the input, the key
    kernel leaves the pair, and the result is the SSG_MSW_KEYS=0 run's"""
    R, idx = world(lib, oracle)
    pes = pes_array(FR)
    x = rescued_hit(lib, oracle, drop_pair(R), pes)
    ties = dict(same_re=region(x["re"] - 40, x["re"], x["qe"] - 40, x["qe"], 35), same_score_rb_qb=region(x["rb"], x["re"] - 7, x["qb"], x["qe"] - 7, x["score"]))
    for name, y in ties.items():
        p = drop_pair(R)
        p.lists[1] = [y]
        p.add_decoys(1, 12, first=600, rest=10)
        try:   # (a region that shares x's (score, rb, qb) and is dropped by the scan before the second sort leaves no tie behind: then the reference holds too)
            want = reference(oracle, R, lib, [p], pes)[0]
        except MR.Tie:
            want = None
        assert name != "same_re" or want is None
        got, err, cnt = same_as_old(lib, idx, [p], pes, monkeypatch)
        assert int(cnt[3]) == 1 and int(cnt[2]) == 0 and not err.any(), (name, cnt)
        if want is not None:
            same_lists(got, want, name)


def case_whole_path(lib, oracle, prefix, monkeypatch):
    """the pipeline with the switch on and off: SAM text equal to the oracle's both times (common.check_pe_sam asserts it), stats equal, and the key kernel
    decided the pipeline's own pairs (ssg_dbg_matesw_last: the counts of the rescue stage of the call just made).  How many it must decide: every reason to
    leave a pair is an exception (a tie of two regions, a window whose skip decision an earlier rescue of the same pair changed, a capacity), so a batch in
    which it leaves half of the listed pairs is the quiet fall-back this test is there to rule out: more than half, and at least one, on both batches."""
    batches = (dict(n_pairs=1500, seed=31, prefix=prefix), dict(n_pairs=300, seed=32, read_len=250, ins_mean=800, ins_std=150))
    res = {}
    for keys in ("1", "0"):
        monkeypatch.setenv("SSG_MSW_KEYS", keys)
        res[keys] = []
        for b in batches:
            text, stats = common.check_pe_sam(lib, oracle, **b)
            cnt = [int(x) for x in lib.dbg_matesw_last()]
            print("SSG_MSW_KEYS=%s, %d pairs: %d listed, %d decided on keys, %d left with %d of %d windows" % (keys, b["n_pairs"], cnt[4], cnt[2], cnt[3], cnt[6], cnt[0]))
            assert cnt[0] == int(stats[3]) and cnt[1] == cnt[0] and cnt[2] + cnt[3] == cnt[4] and cnt[4] > 0, cnt
            if keys == "1":
                assert cnt[2] > 0 and 2 * cnt[2] > cnt[4], "the key kernel left %d of %d listed pairs of the pipeline's batch to ssg_k_matesw" % (cnt[3], cnt[4])
                assert cnt[6] <= cnt[0] and (cnt[3] > 0 or cnt[6] == 0), cnt
            else:
                assert cnt[2] == 0 and cnt[6] == cnt[0], cnt
            res[keys].append((text, stats))
    for (t1, s1), (t0, s0) in zip(res["1"], res["0"]):
        assert t1 == t0 and np.array_equal(s1, s0), (s1, s0)
    assert int(res["1"][0][1][3]) > 10000, "the repeat batch is meant to rescue more than 10 000 windows"
    monkeypatch.delenv("SSG_MSW_KEYS", raising=False)


# ---- the emulator
def test_lengths_fixed_emu(emu_lib, oracle, monkeypatch):
    case_lengths(emu_lib, oracle, monkeypatch, 1)


def test_lengths_unfixed_emu(emu_lib, oracle, monkeypatch):
    case_lengths(emu_lib, oracle, monkeypatch, 0)


def test_too_long_emu(emu_lib, oracle, monkeypatch):
    case_too_long(emu_lib, oracle, monkeypatch)


def test_both_sides_emu(emu_lib, oracle, monkeypatch):
    case_both_sides(emu_lib, oracle, monkeypatch)


def test_drops_emu(emu_lib, oracle, monkeypatch):
    case_drops(emu_lib, oracle, monkeypatch)


def test_leftover_emu(emu_lib, oracle, monkeypatch):
    case_leftover(emu_lib, oracle, monkeypatch)


def test_ties_emu(emu_lib, oracle, monkeypatch):
    case_ties(emu_lib, oracle, monkeypatch)


def test_whole_path_emu(emu_lib, oracle, repeat_pe_prefix, monkeypatch):
    case_whole_path(emu_lib, oracle, repeat_pe_prefix, monkeypatch)


# ---- the device
@pytest.mark.gpu
def test_lengths_fixed_gpu(gpu_lib, oracle, monkeypatch):
    case_lengths(gpu_lib, oracle, monkeypatch, 1)


@pytest.mark.gpu
def test_lengths_unfixed_gpu(gpu_lib, oracle, monkeypatch):
    case_lengths(gpu_lib, oracle, monkeypatch, 0)


@pytest.mark.gpu
def test_too_long_gpu(gpu_lib, oracle, monkeypatch):
    case_too_long(gpu_lib, oracle, monkeypatch)


@pytest.mark.gpu
def test_both_sides_gpu(gpu_lib, oracle, monkeypatch):
    case_both_sides(gpu_lib, oracle, monkeypatch)


@pytest.mark.gpu
def test_drops_gpu(gpu_lib, oracle, monkeypatch):
    case_drops(gpu_lib, oracle, monkeypatch)


@pytest.mark.gpu
def test_leftover_gpu(gpu_lib, oracle, monkeypatch):
    case_leftover(gpu_lib, oracle, monkeypatch)


@pytest.mark.gpu
def test_ties_gpu(gpu_lib, oracle, monkeypatch):
    case_ties(gpu_lib, oracle, monkeypatch)


@pytest.mark.gpu
def test_whole_path_gpu(gpu_lib, oracle, repeat_pe_prefix, monkeypatch):
    case_whole_path(gpu_lib, oracle, repeat_pe_prefix, monkeypatch)
