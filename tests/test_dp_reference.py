"""The three Smith-Waterman operations against a reference that shares nothing with the oracle (tests/dp_reference.py: full-matrix DP for the local and
the global alignment, a second restatement of SURVEY Appendix B's pseudo-code for the extension).

Three layers, the same scoring sets and the same fixed shapes in each:
  * the oracle (oracle/orc_ksw.c) against the reference, on the CPU: what pins the oracle itself;
  * the host-emulation build of the kernel sources against the reference and the oracle, on the CPU;
  * every kernel form on the MI355X against both (`-m gpu`).
The rules are conditions, not tolerances (common.ref_check_*): extension -- score, qle, tle, max_off equal, gscore equal or both <= 0, gtle
equal where gscore > 0; local -- score is the maximum of the reference's H, H[te][qe] holds it, the global alignment of the reported
substrings earns it; global -- the score is the banded optimum and the CIGAR consumes both sequences, stays in the band and earns that
score.  ksw_align2's score2 / te2 and the tie order of ksw_global2's backtrace have no definition outside upstream's code: those stay pinned
to the oracle alone.  Every test asserts that the `gscore <= 0' rule left gtle uncompared on fewer than one in ten of its jobs."""
import numpy as np
import pytest

import common
import dp_reference as R
from speedseq_amd import capi

# (a, b, o_del, e_del, o_ins, e_ins).  The gap penalties of the large match scores are scaled with them, so that gaps stay a decision.
SCORES = [
    (1, 4, 6, 1, 6, 1),        # the default
    (2, 5, 7, 2, 9, 1),        # the set of the CLI tests
    (1, 4, 6, 1, 12, 2),       # insertions dearer than deletions ...
    (1, 4, 12, 2, 6, 1),       # ... and the other way round: swapped penalties show
    (3, 0, 5, 1, 5, 1),        # b == 0
    (1, 4, 40, 3, 40, 3),      # a gap open above most scores
    (15, 16, 30, 5, 36, 4),    # the last scoring the mate-rescue lane kernel takes (a <= 15, b <= 16)
    (16, 16, 30, 5, 36, 4),    # one past it in a: the wave form
    (15, 17, 30, 5, 36, 4),    # one past it in b: the wave form
    (31, 32, 60, 9, 70, 8),    # the edge of the extension lane kernel's 6-bit score table
]
LANE_REFUSES = {(16, 16, 30, 5, 36, 4), (15, 17, 30, 5, 36, 4), (31, 32, 60, 9, 70, 8)}   # beyond k_mswlane.h's 5-bit table: from_lane == 0
END_BONUS = (0, 5, 17)
IDS = ["-".join(str(x) for x in s) for s in SCORES]


def _random_case(rng, k):
    ql, tl = int(rng.integers(1, 14)), int(rng.integers(1, 16))
    q = rng.integers(0, 5, size=ql, dtype=np.uint8)
    t = rng.integers(0, 4, size=tl, dtype=np.uint8)
    if rng.random() < 0.6:
        t = np.array([c for c in common.mutate(rng, q, 3, 2) if c < 4] or [0], dtype=np.uint8)
    return q, t, SCORES[k % len(SCORES)]


def test_vector_rows_equal_the_three_loops():
    """the running-maximum form of F (and the row-at-a-time E, H) against the plain loops, all three operations"""
    rng = np.random.default_rng(5)
    for k in range(400):
        q, t, sc = _random_case(rng, k)
        w, zd, h0, eb = int(rng.choice([1, 2, 5, 100])), int(rng.choice([0, 5, 100])), int(rng.integers(1, 40)) * sc[0], int(rng.choice(END_BONUS))
        (a, am), (b, bm) = R.extend(q, t, sc, w, eb, zd, h0, matrices=True), R.extend_scalar(q, t, sc, w, eb, zd, h0, matrices=True)
        assert a == b and all(np.array_equal(x, y) for x, y in zip(am, bm)), (k, q, t, sc, w, eb, zd, h0, a, b)
        assert np.array_equal(R.local(q, t, sc), R.local_scalar(q, t, sc)), (k, q, t, sc)
        wg = abs(len(q) - len(t)) + int(rng.integers(0, 4))
        assert R.global_(q, t, sc, wg) == R.global_scalar(q, t, sc, wg), (k, q, t, sc, wg)


def test_reference_on_cases_worked_by_hand():
    d = (1, 4, 6, 1, 6, 1)
    q = np.array([0, 1, 2, 3, 0, 1], dtype=np.uint8)
    # a perfect target: every diagonal step adds a; the extension ends at the end of both, to-end score the same
    assert R.extend(q, q, d, 100, 5, 100, 10) == (16, 6, 6, 6, 16, 0)
    # a mismatch at the third base: 10 + 2 = 12 before it, 12 - 4 + 3 = 11 at the end of the query -- the local end wins, the to-end score is 11
    t = q.copy(); t[2] = 0
    assert R.extend(q, t, d, 100, 5, 100, 10) == (12, 2, 2, 6, 11, 0)
    # a target that matches nowhere: the first row is dead, nothing is extended, the anchor's score stays
    assert R.extend(np.zeros(5, dtype=np.uint8), np.full(5, 1, dtype=np.uint8), d, 100, 5, 100, 1)[:3] == (1, 0, 0)
    # local: the common substring of length 4 scores 4 wherever it sits
    H = R.local(np.array([3, 3, 0, 1, 2, 3], dtype=np.uint8), np.array([1, 1, 0, 1, 2, 3, 0], dtype=np.uint8), d)
    assert H.max() == 4 and H[6][6] == 4
    # global: one deleted target base costs o_del + e_del; swapped penalties would give 5 - 14
    assert R.global_(q, np.array([0, 1, 2, 2, 3, 0, 1], dtype=np.uint8), (1, 4, 6, 1, 12, 2), 3) == 6 - 7
    assert R.global_(np.array([0, 1, 2, 2, 3, 0, 1], dtype=np.uint8), q, (1, 4, 6, 1, 12, 2), 3) == 6 - 14
    assert R.rescore([(0, 3), (2, 1), (0, 3)], q, np.array([0, 1, 2, 2, 3, 0, 1], dtype=np.uint8), d) == (6 - 7, 6, 7, 1)
    assert R.global_(q, q, d, 0) == 6 and R.global_(q[:1], q[:1], d, 3) == 1


class _OracleAsLib:
    """the oracle behind the three stage-level calls of capi.Lib that take their sequences directly: common.check_extend / check_local / check_global then
    compare the oracle with the reference through the very code that compares the kernels with it (the lane entry points run the same operations on targets
    read from an index; the oracle has no such form)"""
    def __init__(self, oracle):
        self.o = oracle

    def opt_init(self):
        return np.zeros(1, dtype=capi.OPT_DT)

    def _opt(self, opt):
        s = tuple(int(opt[k][0]) for k in ("a", "b", "o_del", "e_del", "o_ins", "e_ins"))
        return self.o.opt_scores(*s) if any(s) else None

    def extend_batch(self, opt, jobs, qbuf, tbuf):
        oo = self._opt(opt)
        res = np.zeros(len(jobs), dtype=capi.EXT_RES_DT)
        for i, j in enumerate(jobs):
            res[i] = self.o.extend2(np.ascontiguousarray(qbuf[j["qoff"]:j["qoff"] + j["qlen"]]), np.ascontiguousarray(tbuf[j["toff"]:j["toff"] + j["tlen"]]),
                                    int(j["w"]), int(j["end_bonus"]), int(j["zdrop"]), int(j["h0"]), oo)
        return res, 1

    def align2_batch(self, opt, jobs, qbuf, tbuf):
        oo = self._opt(opt)
        res = np.zeros(len(jobs), dtype=capi.KSWR_DT)
        for i, j in enumerate(jobs):
            res[i] = self.o.align2(np.ascontiguousarray(qbuf[j["qoff"]:j["qoff"] + j["qlen"]]), np.ascontiguousarray(tbuf[j["toff"]:j["toff"] + j["tlen"]]), int(j["xtra"]), oo)
        return res

    def global_batch(self, opt, jobs, qbuf, tbuf, cap=64):
        oo = self._opt(opt)
        sc, nc, cg = np.zeros(len(jobs), dtype=np.int32), np.zeros(len(jobs), dtype=np.int32), np.zeros((len(jobs), cap), dtype=np.uint32)
        for i, j in enumerate(jobs):
            sc[i], nc[i], cg[i] = self.o.global2(np.ascontiguousarray(qbuf[j["qoff"]:j["qoff"] + j["qlen"]]), np.ascontiguousarray(tbuf[j["toff"]:j["toff"] + j["tlen"]]), int(j["w"]), cap=cap, opt=oo)
        return sc, nc, cg


def _scores_or_none(scores):
    return None if scores == SCORES[0] else scores   # the default set runs through opt_init() untouched, as the product does


# ---------------------------------------------------------------- CPU: the oracle against the reference
@pytest.mark.parametrize("scores", SCORES, ids=IDS)
def test_oracle_against_reference(oracle, scores):
    lib = _OracleAsLib(oracle)
    tally = common.RefTally()
    for k, eb in enumerate(END_BONUS):
        common.check_extend(lib, oracle, 30, seed=300 + k, max_qlen=318, scores=scores, end_bonus=eb, ref=tally, fixed=True)
    common.check_local(lib, oracle, 12, seed=310, scores=scores, ref=tally, fixed=True)
    common.check_global(lib, oracle, 20, seed=320, scores=scores, ref=tally, fixed=True)
    tally.check_share()


def test_oracle_against_reference_default_scoring_random_jobs(oracle):
    """the batches of the existing kernel tests' generators at their own seeds, default scoring"""
    lib = _OracleAsLib(oracle)
    tally = common.RefTally()
    common.check_extend(lib, oracle, 400, seed=11, ref=tally)
    common.check_local(lib, oracle, 60, seed=12, ref=tally)
    common.check_global(lib, oracle, 150, seed=13, ref=tally)
    tally.check_share()


# ---------------------------------------------------------------- CPU: the emulator build against the reference
QCAPS = (72, 136, 256, 320)


def _kernels_against_reference(lib, oracle, tmp_path, scores, n_ext, n_lane, n_loc, n_glb, lanes, seed):
    """the call list shared by the emulator's test and the GPU's: every end_bonus through extend_batch and through extend_lane_batch at all four qcaps, the
    fixed shapes behind the random jobs of every batch; returns the tally"""
    sc = _scores_or_none(scores)
    tally = common.RefTally()
    for k, eb in enumerate(END_BONUS):
        common.check_extend(lib, oracle, n_ext, seed=seed + k, max_qlen=318, scores=sc, end_bonus=eb, ref=tally, fixed=True)
        common.check_extend_lane(lib, oracle, n_lane, seed=seed + 10 + k, workdir=tmp_path, qcaps=QCAPS, scores=sc, end_bonus=eb, ref=tally, fixed=True)
    common.check_local(lib, oracle, n_loc, seed=seed + 20, scores=sc, ref=tally, fixed=True)
    refuses = scores in LANE_REFUSES
    done, taken = common.check_local_lane(lib, oracle, n_loc, seed=seed + 30, workdir=tmp_path, lanes=lanes, scores=sc, ref=tally, fixed=True, expect_lane=not refuses)
    assert (taken == 0) if refuses else (taken > done // 2), (scores, done, taken)
    common.check_global(lib, oracle, n_glb, seed=seed + 40, scores=sc, ref=tally, fixed=True)
    tally.check_share()
    print("reference: %d jobs (%d extensions, gtle uncompared on %d) in %.1f s" % (tally.jobs, tally.ext_jobs, tally.gtle_excluded, tally.seconds))
    return tally


@pytest.mark.parametrize("scores", SCORES, ids=IDS)
def test_emu_kernels_against_reference(emu_lib, oracle, tmp_path, scores):
    _kernels_against_reference(emu_lib, oracle, tmp_path, scores, n_ext=4, n_lane=2, n_loc=4, n_glb=6, lanes=(4, 1), seed=400)


def _gate_jobs(h0_sum, a, end_bonus, qlen=100):
    """one extension whose h0 + qlen * a + end_bonus is h0_sum"""
    rng = np.random.default_rng(7)
    q = rng.integers(0, 4, size=qlen, dtype=np.uint8)
    t = np.concatenate([q[:60], rng.integers(0, 4, size=70, dtype=np.uint8)])
    jobs = np.array([(0, qlen, 0, t.size, 100, end_bonus, 100, h0_sum - qlen * a - end_bonus)], dtype=capi.EXT_JOB_DT)
    return jobs, q, t


def _host_gates(lib, oracle, tmp_path):
    """each host gate gives a correct result at its limit and SSG_EINVAL one step past it"""
    fa = str(tmp_path / "gate.fa")
    for scores, eb in (((1, 4, 6, 1, 6, 1), 5), ((31, 32, 60, 9, 70, 8), 17), ((2, 5, 7, 2, 9, 1), 0)):
        opt, oopt = common.scored_opts(lib, oracle, scores)
        jobs, q, t = _gate_jobs(8190, scores[0], eb)
        pad = np.random.default_rng(8).integers(0, 4, size=3000)   # the job's target opens a reference of ordinary size
        with open(fa, "w") as f:
            f.write(">t\n" + "".join("ACGT"[c] for c in np.concatenate([t, pad])) + "\n")
        idx = lib.index_build_fasta(fa)
        tally = common.RefTally()
        for qcap in (136, 320):
            res, _ = lib.extend_lane_batch(idx, opt, jobs, np.zeros(1, dtype=np.int64), 1, q, qcap)
            got = tuple(int(x) for x in res[0])
            o = oracle.extend2(q, t, 100, eb, 100, int(jobs[0]["h0"]), oopt)
            assert got == o, ("extend_lane_batch at the ceiling of its cells disagrees with the oracle", scores, qcap, got, o)
            common.ref_check_extend(got, q, t, scores, 100, eb, 100, int(jobs[0]["h0"]), tally, "extend_lane_batch at the ceiling of its cells", (scores, qcap))
            assert got[0] > 8190 - eb - 100 * scores[0] + 50 * scores[0]   # the 60 matching bases were extended: the cells did hold scores near 2^13
        jobs["h0"] += 1                                                      # the sum is 8191: refused, not run
        with pytest.raises(capi.SsgError, match="13-bit"):
            lib.extend_lane_batch(idx, opt, jobs, np.zeros(1, dtype=np.int64), 1, q, 136)
        lib.index_destroy(idx)
    # the aligner's own gate: a <= 31 and b <= 32 run (the kernel tests above), a = 32 or b = 33 is an error return
    gidx = lib.index_load(common.EXAMPLE_FA)
    _, _, seq, off = common.sim_reads(4, seed=3, read_len=100)
    for a, b, ok in ((31, 32, True), (32, 32, False), (31, 33, False)):
        opt, _ = common.scored_opts(lib, None, (a, b, 60, 9, 70, 8))
        if ok:
            capi.mem_process_pairs(lib, gidx, opt, seq, off, id0=0).close()
        else:
            with pytest.raises(capi.SsgError, match="6-bit"):
                capi.mem_process_pairs(lib, gidx, opt, seq, off, id0=0)
    lib.index_destroy(gidx)


def test_emu_host_gates(emu_lib, oracle, tmp_path):
    _host_gates(emu_lib, oracle, tmp_path)


# ---------------------------------------------------------------- MI355X: every kernel form against the reference
@pytest.mark.gpu
@pytest.mark.parametrize("scores", SCORES, ids=IDS)
def test_gpu_kernels_against_reference(gpu_lib, oracle, tmp_path, scores):
    """extend_batch (the wave form); extend_lane_batch at qcaps 72 / 136 / 256 / 320, each with the four reference walks; align2_batch; align2_lane_batch with
    1 / 2 / 4 lanes on both strands -- in the lane kernel up to (15, 16), through the wave form past it --; global_batch"""
    _kernels_against_reference(gpu_lib, oracle, tmp_path, scores, n_ext=12, n_lane=4, n_loc=6, n_glb=20, lanes=(1, 2, 4), seed=400)


@pytest.mark.gpu
def test_gpu_host_gates(gpu_lib, oracle, tmp_path):
    _host_gates(gpu_lib, oracle, tmp_path)
