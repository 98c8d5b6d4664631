"""Seeding intervals (mem_collect_intv) and seed positions (bwt_sa, bns_intv2rid, the max_occ sub-sampling) against a reference that shares nothing with the
oracle or the kernels (tests/seed_reference.py: a suffix array of the doubled text by sorting, occurrence ranges by binary search over text slices, the
three passes from their definitions).

Layers, the same reads and the same six option sets in each:
  * the reference against itself: a twin without the suffix array on random tiny texts, cases worked by hand, every 32nd row against the golden .sa file;
  * the oracle (oracle/orc_mem.c, orc_index.c) against the reference, on the CPU: what pins the oracle itself;
  * the host-emulation build of the kernel sources against the reference, on the CPU;
  * every kernel form on the MI355X against the reference (`-m gpu`).
The comparison is exact equality of the whole list of every read (common.ref_check_smem / ref_check_seeds): x0, x1, x2, info, the count, and for the
seeds rbeg, qbeg, len, rid in order.  No tolerance and no read left out: the tally asserts that every submitted read was compared, and, from the
reference alone, that passes 2 and 3 both produced intervals, that the planted families put x2 on both sides of every threshold, and that seeds
with rid < 0 were seen.

Cost, measured 2026-10-17 on a CPU-only build host (x86-64, one core): the reference takes 2 to 5 ms per read (suffix array: 0.4 s for the golden slice,
once); the not-gpu part of this module takes 10 s.  The reference's lists are made once per (text, option set) and shared by every layer and kernel form.
"""
import ctypes as C

import numpy as np
import pytest

import common
import seed_reference as R
from speedseq_amd import capi

# (min_seed_len, split_factor, split_width, max_occ, max_mem_intv); None: the option blocks as opt_init() leaves them
OPTSETS = [
    None,                           # the defaults: 19, 1.5, 10, 500, 20
    (10, 1.5, 10, 500, 20),         # -k 10: at or below the K of the table of short-pattern intervals (ssg_seed.cpp: min(ktab_k, min_seed_len - 1))
    (32, 1.0, 10, 500, 20),         # -k 32 -r 1.0: every kept match is re-seeded
    (19, 3.0, 10, 500, 0),          # -r 3.0 -y 0: no third pass
    (19, 1.5, 1, 20, 100),          # -c 20 -y 100, split_width 1
    (19, 1.5, 50, 500, 20),         # split_width 50
]
OPT_IDS = ["defaults", "k10", "k32-r1", "r3-y0", "c20-y100-sw1", "sw50"]
CAP = 128          # room for every list of the shared reads


# ---------------------------------------------------------------- the reference against itself
def test_twin_on_random_tiny_texts():
    """suffix array, rank and occ against sorted() over Python strings and a sliding window: 2- and 4-letter alphabets, 30 to 200 bases (doubled: 60 to 400)"""
    rng = np.random.default_rng(1)
    for it in range(60):
        n = int(rng.integers(30, 201))
        fwd = rng.integers(0, 4, size=n).astype(np.uint8) if it % 2 else (rng.integers(0, 2, size=n) * 3).astype(np.uint8)   # A / T only: repeats and self-complements abound
        sr = R.SeedRef(fwd)
        assert sr.sa == R.suffix_array_plain(sr.t2), it
        for _ in range(30):
            m = int(rng.integers(1, 14))
            if rng.random() < 0.7:
                s = int(rng.integers(0, sr.n - m + 1))
                p = sr.t2[s:s + m]
            else:
                p = rng.integers(0, 4, size=m)
            assert sr.occ(p) == R.occ_plain(sr.t2, p) and sr.rank(p) == R.rank_plain(sr.t2, p), (it, list(fwd), list(p))
        assert sr.occ([0, 4, 0]) == 0


def _codes(s):
    return np.array(["ACGT".index(c) for c in s], dtype=np.uint8)


def test_reference_on_cases_worked_by_hand():
    # fwd = ACG: T2 = ACGCGT.  Suffixes sorted: ACGCGT(0) CGCGT(1) CGT(3) GCGT(2) GT(4) T(5)
    sr = R.SeedRef(_codes("ACG"))
    assert sr.sa == [0, 1, 3, 2, 4, 5]
    # CG is its own reverse complement: two suffixes start with it, one sorts before it: x0 == x1 == 2, x2 == 2
    assert sr.interval(_codes("CG"), 0, 2) == (2, 2, 2, 2)
    # ACG: nothing sorts before it, x0 = 1; its reverse complement CGT has two suffixes before it (ACGCGT, CGCGT), x1 = 3; info = 0 << 32 | 3
    assert sr.interval(_codes("ACG"), 0, 3) == (1, 3, 1, 3)
    # GT runs to the last base of T2, and T alone is the shortest suffix: it sorts before everything that would extend it
    assert sr.occ(_codes("GT")) == 1 and sr.rank(_codes("T")) == 5 and sr.occ(_codes("TA")) == 0 and sr.rank(_codes("TA")) == 6
    # GCG occurs only across the strand junction (fwd ends ..CG, the reverse strand begins CG..): position 2 covers bases 2, 3, 4 with l_pac = 3
    assert sr.occ(_codes("GCG")) == 1 and sr.sa[sr.rank(_codes("GCG"))] == 2 and sr.rid(2, 3) == -2 and sr.rid(0, 3) == 0 and sr.rid(3, 3) == 0
    # a tandem repeat: fwd = ACACACAC, T2 = ACACACAC GTGTGTGT; ACAC occurs at 0, 2, 4; CACA at 1, 3; the read ACACAC has one supermaximal match, itself, twice
    sr = R.SeedRef(_codes("ACACACAC"))
    assert sr.occ(_codes("ACAC")) == 3 and sr.occ(_codes("CACA")) == 2 and sr.occ(_codes("GTGT")) == 3
    o = R.SeedOpts(3, 1.5, 1, 500, 0)            # split_width 1 < x2: no re-seeding
    assert sr.collect_intv(_codes("ACACAC"), o) == [sr.interval(_codes("ACACAC"), 0, 6)] and sr.interval(_codes("ACACAC"), 0, 6)[2] == 2
    # the same read with split_len (int)(3 * 1.0 + .499) = 3: the match (0, 6), x2 = 2 <= split_width, is re-seeded from x = 3 with m = 3: ACAC occurs 3 times,
    # ACACA and CACA twice; the matches through base 3 that keep 3 occurrences and cannot grow either way are ACAC at (0, 4) and ACAC at (2, 6)
    o = R.SeedOpts(3, 1.0, 10, 500, 0)
    got, ps = sr.collect_intv(_codes("ACACAC"), o, passes=True)
    assert ps == (1, 2, 0) and [t[3] for t in got] == [0 << 32 | 4, 0 << 32 | 6, 2 << 32 | 6] and [t[2] for t in got] == [3, 2, 3]
    # two contigs AC | GT (offsets 0, 2): T2 = ACGT ACGT.  CG at 1 spans the contigs (-1), at 5 it does so on the other strand (-1); AC at 0 lies in contig 0,
    # AC at 4 is the reverse strand of GT: contig 1; GTAC at 2 spans the junction (-2)
    sr = R.SeedRef(_codes("ACGT"), [0, 2], [2, 2])
    assert [sr.rid(1, 2), sr.rid(5, 2), sr.rid(0, 2), sr.rid(4, 2), sr.rid(2, 4), sr.rid(6, 2)] == [-1, -1, 0, 1, -2, 0]
    # third pass: min_seed_len 2, max_mem_intv 2, read ACGTAC on that text: from x = 0 the first i with i - x >= 2 is 2: ACG occurs twice (not < 2); i = 3: ACGT twice;
    # i = 4: ACGTA once: kept as (0, 5); from x = 5: C, the read runs out
    got, ps = sr.collect_intv(_codes("ACGTAC"), R.SeedOpts(2, 9.0, 0, 500, 2), passes=True)
    assert ps[2] == 1 and (0 << 32 | 5) in [t[3] for t in got] and sr.occ(_codes("ACGT")) == 2 and sr.occ(_codes("ACGTA")) == 1
    # the sub-sampling: x2 = 7, max_occ 3: step 2, rows k = 0, 2, 4
    sr = R.SeedRef(_codes("ACCACCACCACCACCACCACC"))
    iv = sr.interval(_codes("ACC"), 0, 3)
    assert iv[2] == 7 and [s[0] for s in sr.seeds_of([iv], R.SeedOpts(3, 1.5, 10, 3, 0))] == [sr.sa[iv[0] - 1 + k] for k in (0, 2, 4)]


def test_suffix_array_against_the_golden_sa_file():
    """every 32nd row of the reference's suffix array equals the samples of tests/golden/chr20_slice.fa.sa, and the file's header words (primary, L2, the
    interval, the length) are what the reference's text gives: bytes the reference tree holds"""
    sr = common.seed_ref(common.EXAMPLE_FA)
    w = np.fromfile(common.EXAMPLE_FA + ".sa", dtype=np.uint64)
    primary, L2, intv, seq_len = int(w[0]), [int(x) for x in w[1:5]], int(w[5]), int(w[6])
    assert intv == 32 and seq_len == sr.n == 643270
    assert primary == sr.sa.index(0) + 1                                   # the row of the whole text, behind the sentinel's
    assert L2 == [int(x) for x in np.cumsum(np.bincount(sr.t2, minlength=4))]
    samples = w[7:].astype(np.int64)
    assert samples.size == (seq_len + intv) // intv - 1                    # row 0 (the sentinel) is not stored
    assert np.array_equal(samples, sr.sa_np[intv - 1::intv][:samples.size])   # row r >= 1 of the BWT matrix is SA[r - 1]


# ---------------------------------------------------------------- shared texts, reads and reference lists
@pytest.fixture(scope="module")
def planted(oracle, tmp_path_factory):
    return common.planted_reference(oracle, tmp_path_factory.mktemp("planted"))


_READS, _LISTS = {}, {}


def _reads(prefix, meta, many=False):
    if prefix not in _READS:
        _READS[prefix] = common.fixed_seed_reads(common.seed_ref(prefix), seed=3, planted=meta, n_sim=24, fasta=prefix)
    return [r for r in _READS[prefix] if many == r[0].startswith("many")]


def _lists(prefix, meta, k):
    """the reference's lists of the shared reads, once per (text, option set)"""
    if (prefix, k) not in _LISTS:
        seqs, _, _ = common.cat_reads(_reads(prefix, meta))
        _LISTS[prefix, k] = common.seed_reference_lists(common.seed_ref(prefix), seqs, R.SeedOpts(*OPTSETS[k]) if OPTSETS[k] else R.DEFAULTS)
    return _LISTS[prefix, k]


def _text(which, planted):
    return (common.EXAMPLE_FA, None) if which == "golden" else planted


def _check_tally(tally, k, is_planted, seeds):
    tally.check(passes=False)
    third = (OPTSETS[k] or R.DEFAULTS)[4] > 0
    assert tally.pass2 > 0 and (tally.pass3 > 0) == third, ("reads with intervals of pass 2 / pass 3", tally.pass2, tally.pass3)
    if not is_planted:
        return
    if seeds:
        assert tally.neg_rid > 0, "no seed with rid < 0 among %d" % tally.seeds
    want = set(common.PLANTED_FAMILIES) if (OPTSETS[k] or R.DEFAULTS)[0] <= 30 else {10, 11, 19, 20, 21, 39, 40, 41, 100}   # (the large families are 30 bases long)
    assert want <= tally.x2, ("a planted family drifted off its count", sorted(want - tally.x2))


def _against_reference(run_smem, run_seeds, prefix, meta, k, who):
    """run_smem(seq, off) -> (intv, cnt); run_seeds(seq, off) -> (seed_off, seeds, rids): every read's lists against the reference's"""
    reads = _reads(prefix, meta)
    seqs, seq, off = common.cat_reads(reads)
    want = _lists(prefix, meta, k)
    sref = common.seed_ref(prefix)
    t1, t2 = common.SeedTally(), common.SeedTally()
    intv, cnt = run_smem(seq, off)
    for r, (name, _) in enumerate(reads):
        common.ref_check_smem(intv[r][:cnt[r]], seqs[r], None, sref, t1, who, (prefix, OPT_IDS[k], name), want=want[r])
    seed_off, seeds, rids = run_seeds(seq, off)
    for r, (name, _) in enumerate(reads):
        lo, hi = int(seed_off[r]), int(seed_off[r + 1])
        common.ref_check_seeds(seeds[lo:hi], rids[lo:hi], seqs[r], None, sref, t2, who, (prefix, OPT_IDS[k], name), want=want[r])
    assert t1.submitted == t2.submitted == len(reads)
    _check_tally(t1, k, meta is not None, False)
    _check_tally(t2, k, meta is not None, True)
    return t1, t2


def test_planted_families_hit_every_threshold_from_both_sides(planted):
    """from the reference alone: the families occur exactly as often as planted; at the defaults a family of 10 is re-seeded and one of 11 is not; the third
    pass stops at 20 bases in a family of 19 and runs on in families of 20 and 21; with -c 20 the steps are 1, 1, 1, 2, 2, 5 and no interval gives more than 20 seeds"""
    prefix, meta = planted
    sr = common.seed_ref(prefix)
    assert len(sr.ctg_len) == 3 and 30000 < sr.l_pac < 200000
    for k, F in meta["families"].items():
        assert sr.occ(F) == k and sr.occ(np.concatenate([[0], F, [0]])) == k, k
    assert sr.interval(meta["selfrc"], 0, 60)[0] == sr.interval(meta["selfrc"], 0, 60)[1] and sr.occ(meta["selfrc"]) == 2
    reads = dict(_reads(prefix, meta) + _reads(prefix, meta, many=True))
    fam = lambda k, o: sr.collect_intv(reads["family%d" % k], o, passes=True)
    assert fam(10, R.DEFAULTS)[1][1] > 0 and fam(11, R.DEFAULTS)[1][1] == 0                              # x2 <= split_width
    # (F is bases 13 .. 52 of the read; the third pass finds nothing in the first 20 bases and starts again at base 20, inside F)
    third = lambda k: [t for t in fam(k, R.DEFAULTS)[0] if t[3] == (20 << 32 | 40)]
    assert len(third(19)) == 1 and third(19)[0][2] == 19 and not third(20) and not third(21)             # occ < max_mem_intv
    c20 = R.SeedOpts(*OPTSETS[4])
    for k, step in ((20, 1), (21, 1), (39, 1), (40, 2), (41, 2), (100, 5)):
        iv = [t for t in fam(k, c20)[0] if t[2] == k][0]
        sd = sr.seeds_of([iv], c20)
        assert len(sd) == 20 and [s[0] for s in sd] == [sr.sa[iv[0] - 1 + j * step] for j in range(20)], k
    for k, n, step in ((520, 500, 1), (1003, 500, 2)):
        iv = [t for t in fam(k, R.DEFAULTS)[0] if t[2] == k][0]
        sd = sr.seeds_of([iv], R.DEFAULTS)
        assert len(sd) == n and sd[-1][0] == sr.sa[iv[0] - 1 + (n - 1) * step], k
    assert len(sr.collect_intv(reads["many310"], R.DEFAULTS)) > 155 and len(sr.collect_intv(reads["many100"], R.DEFAULTS)) > 64   # beyond the first capacity of ssg_seeds_batch
    assert sr.collect_intv(reads["mm_every10"], R.DEFAULTS) == [] and sr.collect_intv(reads["allN"], R.DEFAULTS) == []
    ex = sr.collect_intv(reads["exact"], R.DEFAULTS, passes=True)
    assert ex[1][0] == 1 and (1, 150) in [(t[2], t[3]) for t in ex[0]]
    runs = [(t[3] >> 32, t[3] & 0xffffffff) for t in sr.collect_intv(reads["runs27_28"], R.SeedOpts(19, 1.5, 10, 500, 0))]
    assert {(0, 27), (28, 56), (57, 84), (85, 113)} <= set(runs)


# ---------------------------------------------------------------- CPU: the oracle against the reference
class _OracleAsLib:
    """the oracle behind smem_batch / seeds_batch of capi.Lib"""
    def __init__(self, oracle, prefix, oopt, cap=CAP):
        self.o, self.idx, self.oopt, self.cap = oracle, oracle.idx_load(prefix), oopt, cap

    def smem(self, seq, off):
        n = len(off) - 1
        intv, cnt = np.zeros((n, self.cap), dtype=capi.INTV_DT), np.zeros(n, dtype=np.int32)
        for r in range(n):
            o = self.o.collect_intv(self.idx, np.ascontiguousarray(seq[off[r]:off[r + 1]]), cap=1 << 14, opt=self.oopt)
            cnt[r] = len(o); intv[r, :len(o)] = o
        return intv, cnt

    def seeds(self, seq, off):
        n = len(off) - 1
        rows = [self.o.seeds(self.idx, np.ascontiguousarray(seq[off[r]:off[r + 1]]), opt=self.oopt) for r in range(n)]
        seed_off = np.zeros(n + 1, dtype=np.int64)
        seed_off[1:] = np.cumsum([len(x) for x in rows])
        al = np.concatenate(rows) if rows else np.zeros((0, 4), dtype=np.int64)
        seeds = np.zeros(len(al), dtype=capi.SEED_DT)
        seeds["rbeg"], seeds["qbeg"], seeds["len"] = al[:, 0], al[:, 1], al[:, 2]
        return seed_off, seeds, al[:, 3].astype(np.int32)


@pytest.mark.parametrize("k", range(len(OPTSETS)), ids=OPT_IDS)
@pytest.mark.parametrize("which", ["golden", "planted"])
def test_oracle_against_reference(oracle, planted, which, k):
    prefix, meta = _text(which, planted)
    _, oopt, _ = common.seed_opts(None, oracle, OPTSETS[k])
    lib = _OracleAsLib(oracle, prefix, oopt)
    _against_reference(lib.smem, lib.seeds, prefix, meta, k, "the oracle")


def test_oracle_against_reference_long_lists(oracle, planted):
    """the read with an interval at every start: about 300 intervals at the defaults, thousands with -k 10 (every one of them re-seeded)"""
    prefix, meta = planted
    sref = common.seed_ref(prefix)
    for k in (0, 1):
        reads, seqs, seq, off, want = _many(prefix, meta, k)
        lib = _OracleAsLib(oracle, prefix, common.seed_opts(None, oracle, OPTSETS[k])[1], cap=1 << 14)
        tally = common.SeedTally()
        intv, cnt = lib.smem(seq, off)
        seed_off, seeds, rids = lib.seeds(seq, off)
        for i in range(len(reads)):
            lo, hi = int(seed_off[i]), int(seed_off[i + 1])
            common.ref_check_smem(intv[i][:cnt[i]], seqs[i], None, sref, tally, "the oracle", (OPT_IDS[k], reads[i][0]), want=want[i])
            common.ref_check_seeds(seeds[lo:hi], rids[lo:hi], seqs[i], None, sref, tally, "the oracle", (OPT_IDS[k], reads[i][0]), want=want[i])
        tally.check(passes=False)
        assert tally.pass3 > 0 and (tally.pass2 > 0) == (k == 1)     # 20-base matches: below split_len at the defaults, above it with -k 10
        assert tally.seeds > 300


# ---------------------------------------------------------------- the kernels against the reference
def _kernels_against_reference(lib, prefix, meta, ks, load=None):
    gidx = load() if load else lib.index_load(prefix)
    for k in ks:
        opt, _, _ = common.seed_opts(lib, None, OPTSETS[k])
        _against_reference(lambda seq, off: lib.smem_batch(gidx, opt, seq, off, cap=CAP), lambda seq, off: lib.seeds_batch(gidx, opt, seq, off), prefix, meta, k, "%s %s" % (lib.backend(), OPT_IDS[k]))
    return gidx


def _many(prefix, meta, k):
    reads = [r for r in _reads(prefix, meta) if r[0] == "exact"] + _reads(prefix, meta, many=True)
    seqs, seq, off = common.cat_reads(reads)
    return reads, seqs, seq, off, common.seed_reference_lists(common.seed_ref(prefix), seqs, R.SeedOpts(*OPTSETS[k]) if OPTSETS[k] else R.DEFAULTS)


def _list_capacities(lib, prefix, meta):
    """the read with an interval at every start.  At the defaults its lists (about 90 and 300 intervals) outgrow the first capacity of ssg_seeds_batch (64, or half
    the longest read): the batch is run again, wider, and equals the reference.  A capacity the caller gives and a list cannot fit is SSG_EOVERFLOW.  With -k 10 every one
    of those intervals is re-seeded and the list passes 8 x the read length, the last capacity there is: SSG_EOVERFLOW again, never a truncated list."""
    gidx = lib.index_load(prefix)
    sref = common.seed_ref(prefix)
    reads, seqs, seq, off, want = _many(prefix, meta, 0)
    assert [len(w[0]) > c for w, c in zip(want, (0, 155, 64))] == [True] * 3
    opt = lib.opt_init()
    tally = common.SeedTally()
    for sel in ((0, 1, 2), (0, 2)):        # with the 310-base read the first capacity is 155, without it 64
        _, sseq, soff = common.cat_reads([reads[i] for i in sel])
        seed_off, seeds, rids = lib.seeds_batch(gidx, opt, sseq, soff)
        for j, i in enumerate(sel):
            lo, hi = int(seed_off[j]), int(seed_off[j + 1])
            common.ref_check_seeds(seeds[lo:hi], rids[lo:hi], seqs[i], None, sref, tally, "seeds_batch, widened", reads[i][0], want=want[i])
    intv, cnt = lib.smem_batch(gidx, opt, seq, off, cap=512)
    for i in range(len(reads)):
        common.ref_check_smem(intv[i][:cnt[i]], seqs[i], None, sref, tally, "smem_batch", reads[i][0], want=want[i])
    tally.check(passes=False)
    with pytest.raises(capi.SsgError, match="error -75"):
        lib.smem_batch(gidx, opt, seq, off, cap=64)
    opt10, _, _ = common.seed_opts(lib, None, OPTSETS[1])
    want10 = _many(prefix, meta, 1)[4]
    assert len(want10[1][0]) > 8 * 310 + 64
    with pytest.raises(capi.SsgError, match="error -75"):
        lib.smem_batch(gidx, opt10, seq, off, cap=512)
    with pytest.raises(capi.SsgError, match="error -75"):
        lib.seeds_batch(gidx, opt10, seq, off)
    lib.index_destroy(gidx)


@pytest.mark.parametrize("which", ["golden", "planted"])
def test_emu_kernels_against_reference(emu_lib, planted, which):
    prefix, meta = _text(which, planted)
    emu_lib.index_destroy(_kernels_against_reference(emu_lib, prefix, meta, range(len(OPTSETS))))


@pytest.mark.parametrize("which", ["golden", "planted"])
def test_emu_table_k_at_and_above_min_seed_len(emu_lib, planted, monkeypatch, which):
    """-k 10 with a table of short-pattern intervals of K = 9, 10 and 11 asked for (the golden slice is worth up to 11, the planted text up to 10): the cap
    min(K, min_seed_len - 1) of ssg_seed.cpp.  Without it the third pass would start K bases in, past the first length it has to look at."""
    prefix, meta = _text(which, planted)
    for K in ("9", "10", "11"):
        monkeypatch.setenv("SSG_KTAB_K", K)
        emu_lib.index_destroy(_kernels_against_reference(emu_lib, prefix, meta, (1,)))


def test_emu_list_capacities(emu_lib, planted):
    _list_capacities(emu_lib, *planted)


FORMS = {
    "default": {},
    "wave-kernel-all-reads": {"SSG_SMEM_MAX_EXT": "1"},
    "ext700-row18": {"SSG_SMEM_MAX_EXT": "700", "SSG_SMEM_MAX_ROW": "18"},
    "lane-fallback": {"SSG_SMEM_KERNEL": "lane"},
    "ktab0": {"SSG_KTAB_K": "0", "SSG_KTAB_VERIFY": "1"},
    "ktab2": {"SSG_KTAB_K": "2", "SSG_KTAB_VERIFY": "1"},
    "ktab11": {"SSG_KTAB_K": "11", "SSG_KTAB_VERIFY": "1"},
    "ktab25": {"SSG_KTAB_K": "25", "SSG_KTAB_VERIFY": "1"},
    "sa-every-32": {"SSG_SA_INTV": "32"},
}


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["golden", "planted"])
@pytest.mark.parametrize("form", list(FORMS), ids=list(FORMS))
def test_gpu_kernel_forms_against_reference(gpu_lib, planted, monkeypatch, form, which):
    """every form of the seeding kernels (the variables are read at index load and at launch), all six option sets, intervals and seeds"""
    for name, v in FORMS[form].items():
        monkeypatch.setenv(name, v)
    prefix, meta = _text(which, planted)
    gpu_lib.index_destroy(_kernels_against_reference(gpu_lib, prefix, meta, range(len(OPTSETS))))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["golden", "planted"])
def test_gpu_deferred_then_densified_index_against_reference(gpu_lib, planted, which):
    """seeds located through the file's own suffix-array samples (defer_dense_sa), then through the denser copy ssg_index_densify makes of them"""
    prefix, meta = _text(which, planted)

    def load():
        h = C.c_void_p()
        gpu_lib._chk(gpu_lib.l.ssg_index_load2(prefix.encode(), 1, C.byref(h)))
        return h
    gidx = _kernels_against_reference(gpu_lib, prefix, meta, (0, 4), load=load)
    gpu_lib._chk(gpu_lib.l.ssg_index_densify(gidx))
    _kernels_against_reference(gpu_lib, prefix, meta, (0, 4), load=lambda: gidx)
    gpu_lib.index_destroy(gidx)


@pytest.mark.gpu
def test_gpu_list_capacities(gpu_lib, planted):
    _list_capacities(gpu_lib, *planted)
