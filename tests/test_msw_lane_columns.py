"""The mate-rescue lane kernel (k_mswlane.h: both passes of ksw_align2) against the full-matrix reference, result for result.

What the kernel does per cell and per column can go wrong in three places, and the inputs are the smallest that reach them:
  * one `H - (open + extend)' serves E and F when the two sums are equal: the four scorings are the default, one with different sums, one with equal
    sums and different extensions, and -A 2 -B 5;
  * the row maximum of a column pair is folded with one max3, ties to the smaller column: windows whose row maxima are reached in both columns of a
    pair, and in columns of two different lanes of the job (checked below from the reference alone);
  * the reverse pass runs the columns of the wave's longest query, not of its padded length: query lengths 1 .. 33 and 149 .. 153 mixed in one call --
    different real lengths under one padded length in one chunk, 152 against 160 columns at four lanes.
The forward pass keeps upstream's pad columns, and `_pad_jobs' is why: ksw_align2 takes row maxima over the SSE-padded query (zero-scoring columns up to
a multiple of 16 or 8), a pad column k hands the last query column's H of k + 1 rows ago to the row maximum, and the b[] list (score2 / te2) sees it.

The expected result is derived from tests/dp_reference.py's H alone: `_padded' appends the pad columns to it by the same recurrence (plain loops),
`_expect' applies upstream's bookkeeping to the row maxima.  The CPU part also holds that derivation against the oracle."""
import functools
import os

import numpy as np
import pytest

import common
import dp_reference as R
from speedseq_amd import capi

# (a, b, o_del, e_del, o_ins, e_ins)
SCORINGS = [
    (1, 4, 6, 1, 6, 1),    # the default: equal sums
    (1, 4, 7, 2, 9, 1),    # -O 7,9 -E 2,1: different sums
    (1, 4, 7, 1, 6, 2),    # -O 7,6 -E 1,2: equal sums, different extensions
    (2, 5, 6, 1, 6, 1),    # -A 2 -B 5: 16-bit cells (p = 8) from 125 bases on, so 149 .. 152 pad to 152 and 153 to 160
]
IDS = ["-".join(str(x) for x in s) for s in SCORINGS]
QLENS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 33, 149, 150, 151, 152, 153)
WINDOWS = (1, 7, 8, 9, 19, 65, 200)
LANES = (1, 2, 4)


# ---------------------------------------------------------------- the jobs: (query, window as the kernel reads it, on the reverse strand?)
def _base_jobs(rng):
    """every query length against every window length; the window holds a mutated piece of the query where it is long enough to"""
    out = []
    for ql in QLENS:
        for k, w in enumerate(WINDOWS):
            q = rng.integers(0, 4, size=ql, dtype=np.uint8)
            piece = np.array(common.mutate(rng, q[int(rng.integers(0, max(1, ql // 3))):], 3, 2) or [0], dtype=np.uint8)
            lead = int(rng.integers(0, max(1, w - min(w, piece.size) + 1)))
            t = np.concatenate([rng.integers(0, 4, size=lead, dtype=np.uint8), piece, rng.integers(0, 4, size=w, dtype=np.uint8)])[:w]
            if (ql + k) % 5 == 0:
                q = q.copy(); q[int(rng.integers(0, ql))] = 4          # an N in the query
            out.append((q, t, (ql + k) % 2 == 1))
    return out


def _tie_jobs(rng):
    """row maxima reached more than once: runs of one base (every column from the row's own on holds the maximum: both columns of a pair, all lanes),
    and a motif at both ends of the query (the row that ends the motif in the window holds its score in a column below 38 and in one from 120 on:
    the first and the last lane of the job at two and at four lanes, whatever the columns per lane)"""
    out = []
    for ql, w in ((150, 19), (152, 9), (149, 65), (33, 8), (16, 7)):
        q = np.full(ql, 2, dtype=np.uint8)
        t = np.full(w, 2, dtype=np.uint8)
        out.append((q, t, False))
        q2 = q.copy(); q2[ql // 2] = 1
        t2 = t.copy(); t2[w // 2] = 3
        out.append((q2, t2, True))
    for ql in (150, 152, 153):
        m = rng.integers(0, 4, size=24, dtype=np.uint8)
        q = rng.integers(0, 4, size=ql, dtype=np.uint8)
        q[:24] = m; q[ql - 26:ql - 2] = m
        t = np.concatenate([rng.integers(0, 4, size=20, dtype=np.uint8), m, rng.integers(0, 4, size=21, dtype=np.uint8)])
        out.append((q, t, ql == 152))
    return out


def _pad_jobs(rng):
    """a perfect hit, and behind it a second hit that ends in the LAST query column d rows short of te + score, the edge of the stretch that score2
    leaves out: the rows after it hold the second hit's score only in upstream's pad columns, and the b[] entries they make lie past the edge"""
    out = []
    for ql, tail, ds in ((33, 25, (0, 1, 2, 3, 4, 5)), (150, 90, (0, 2, 4))):
        for d in ds:
            q = rng.integers(0, 4, size=ql, dtype=np.uint8)
            gap = ql - tail - d                                          # the second hit ends at row te + ql - d
            t = np.concatenate([rng.integers(0, 4, size=10, dtype=np.uint8), q, 3 - q[ql - tail - gap:ql - tail][::-1], q[ql - tail:], 3 - q[:20]])
            out.append((q, t, d % 2 == 1))
    return out


@functools.lru_cache(maxsize=None)
def _jobs():
    rng = np.random.default_rng(909)
    base, tie, pad = _base_jobs(rng), _tie_jobs(rng), _pad_jobs(rng)
    return base + tie + pad, (len(base), len(base) + len(tie))


# ---------------------------------------------------------------- the expected result, from the reference's H
def _padded(H, scores, p):
    """H of dp_reference.local (boundary row and column 0) with upstream's pad columns appended: query positions qlen .. qp - 1 score 0 against every
    target base.  F of a pad column opens from the H of the row, E from the H of the column, as everywhere."""
    _, _, o_del, e_del, o_ins, e_ins = scores
    tlen, qlen = H.shape[0] - 1, H.shape[1] - 1
    qp = (qlen + p - 1) // p * p
    Hp = np.zeros((tlen + 1, qp + 1), dtype=np.int64)
    Hp[:, :qlen + 1] = H
    if qp == qlen:
        return Hp
    E = [0] * (qp + 1)
    for i in range(1, tlen + 1):
        f = 0
        for k in range(1, qlen + 1):                                     # F entering the first pad column, from the row's H alone
            f = max(f - e_ins, int(Hp[i][k]) - (o_ins + e_ins), 0)
        for j in range(qlen + 1, qp + 1):
            E[j] = max(E[j] - e_del, int(Hp[i - 1][j]) - (o_del + e_del), 0)
            h = max(0, int(Hp[i - 1][j - 1]), E[j], f)
            Hp[i][j] = h
            f = max(f - e_ins, h - (o_ins + e_ins), 0)
    return Hp


def _pass(Hp, minsc, endsc, maxsc):
    """upstream's bookkeeping over the row maxima: (score, te, qe, score2, te2); the pass ends at the row that reaches endsc"""
    body = Hp[1:, 1:]
    gmax, te, qe, b = 0, -1, 0, []
    for i in range(body.shape[0]):
        imax = int(body[i].max())
        if imax >= minsc:
            if not b or b[-1][1] + 1 != i:
                b.append([imax, i])
            elif b[-1][0] < imax:
                b[-1] = [imax, i]
        if imax > gmax:
            gmax, te, qe = imax, i, int(body[i].argmax())               # the smallest column that holds it
            if gmax >= endsc:
                break
    score2, te2 = -1, -1
    if b:
        k = (gmax + maxsc - 1) // maxsc
        for sc, e in b:
            if (e < te - k or e > te + k) and sc > score2:
                score2, te2 = sc, e
    return gmax, te, qe, score2, te2


def _expect(q, t, scores, xtra, pads=True):
    p = 16 if xtra & common.KSW_XBYTE else 8
    minsc = xtra & 0xffff if xtra & common.KSW_XSUBO else 0x10000
    maxsc = max(scores[0], 1)
    H = R.local(q, t, scores)
    score, te, qe, score2, te2 = _pass(_padded(H, scores, p) if pads else H, minsc, 0x10000, maxsc)
    tb = qb = -1
    if (xtra & common.KSW_XSTART) and not ((xtra & common.KSW_XSUBO) and score < (xtra & 0xffff)):
        Hr = R.local(q[:qe + 1][::-1], t[:te + 1][::-1], scores)
        rs, rte, rqe, _, _ = _pass(_padded(Hr, scores, p) if pads else Hr, 0x10000, score, maxsc)
        if rs == score:
            tb, qb = te - rte, qe - rqe
    return (score, te, qe, score2, te2, tb, qb), H


def _ties(H, te):
    """(the row of the result holds its maximum in both columns of a pair, ... in a column below 38 and in one from 120 on)"""
    if te < 0:
        return False, False
    row = H[te + 1][1:]
    at = np.flatnonzero(row == row.max())
    pair = any(c % 2 == 0 and c + 1 in at for c in at)
    return pair, bool(at[0] < 38 and at[-1] >= 120)


@functools.lru_cache(maxsize=None)
def _expected(scores):
    """per job: the expected result with upstream's pad columns; per scoring: what the inputs reach (asserted by the CPU test)"""
    jobs, (n_base, n_tie) = _jobs()
    want, facts = [], dict(rev=0, norev=0, pair=0, lane=0, pad_live=0)
    for i, (q, t, _) in enumerate(jobs):
        xtra = common.local_xtra(len(q), scores)
        w, H = _expect(q, t, scores, xtra)
        want.append(w)
        facts["rev" if _has_rev(w, xtra) else "norev"] += 1
        if n_base <= i < n_tie:
            pair, lane = _ties(H, w[1])
            facts["pair"] += pair; facts["lane"] += lane
        if i >= n_tie and _expect(q, t, scores, xtra, pads=False)[0] != w:
            facts["pad_live"] += 1
    return want, facts


# ---------------------------------------------------------------- the run
def _run(lib, workdir, scores):
    jobs, _ = _jobs()
    want, _ = _expected(scores)
    n = len(jobs)
    rows, qo, to, fasta, tpos = [], 0, 0, [], []
    for q, t, rev in jobs:
        rows.append((qo, len(q), to, len(t), common.local_xtra(len(q), scores), 0))
        fasta.append((3 - t[::-1]) if rev else t)
        tpos.append(to)
        qo += len(q); to += len(t)
    L = to
    tpos = np.array([2 * L - s - len(jobs[i][1]) if jobs[i][2] else s for i, s in enumerate(tpos)], dtype=np.int64)
    fa = os.path.join(str(workdir), "mswcols.fa")
    with open(fa, "w") as f:
        f.write(">t\n")
        txt = "".join("ACGT"[c] for c in np.concatenate(fasta))
        for k in range(0, len(txt), 80):
            f.write(txt[k:k + 80] + "\n")
    idx = lib.index_build_fasta(fa)
    opt, _ = common.scored_opts(lib, None, scores)
    sw = np.array(rows, dtype=capi.SW_JOB_DT)
    qbuf = np.concatenate([q for q, _, _ in jobs])
    for nl in LANES:
        res, from_lane = lib.align2_lane_batch(idx, opt, sw, tpos, qbuf, nl)
        for i in range(n):
            got = tuple(int(x) for x in res[i])
            assert got == want[i], ("the lane kernel disagrees with the full-matrix reference", scores, "lanes", nl, "job", i, "qlen", len(jobs[i][0]), "tlen", len(jobs[i][1]),
                                    "reverse strand", jobs[i][2], "got", got, "reference", want[i], "from_lane", int(from_lane[i]))
            assert int(from_lane[i]) == (2 if _has_rev(want[i], rows[i][4]) else 1), ("a pass of this job did not come from the lane kernel", scores, nl, i, int(from_lane[i]), want[i])
    lib.index_destroy(idx)
    return n * len(LANES)


def _has_rev(w, xtra):
    return bool(xtra & common.KSW_XSTART) and not ((xtra & common.KSW_XSUBO) and w[0] < (xtra & 0xffff))


@pytest.mark.parametrize("scores", SCORINGS, ids=IDS)
def test_reference_derivation_and_what_the_inputs_reach(oracle, scores):
    """the expected results equal the oracle's (the bookkeeping above is upstream's), and the inputs hold what they are there for"""
    jobs, (n_base, n_tie) = _jobs()
    want, facts = _expected(scores)
    _, oopt = common.scored_opts(None, oracle, scores)
    for i, (q, t, _) in enumerate(jobs):
        o = oracle.align2(np.ascontiguousarray(q), np.ascontiguousarray(t), common.local_xtra(len(q), scores), oopt)
        assert o == want[i], ("the derivation from the reference's H disagrees with the oracle", scores, i, len(q), len(t), o, want[i])
    assert len(jobs) <= 200
    assert facts["rev"] >= 20 and facts["norev"] >= 20, facts           # forward scores that call for the reverse pass, and ones that do not
    assert facts["pair"] >= 5 and facts["lane"] >= 3, facts             # the result's row holds its maximum twice: in a column pair, in two lanes
    assert facts["pad_live"] >= 6, facts                                 # without the pad columns the expected result itself would be another


@pytest.mark.parametrize("scores", SCORINGS, ids=IDS)
def test_emu_lane_kernel_exact(emu_lib, tmp_path, scores):
    assert _run(emu_lib, tmp_path, scores) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("scores", SCORINGS, ids=IDS)
def test_gpu_lane_kernel_exact(gpu_lib, tmp_path, scores):
    assert _run(gpu_lib, tmp_path, scores) > 0
