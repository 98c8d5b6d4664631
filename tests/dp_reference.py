"""Independent references of the three Smith-Waterman operations (ksw_extend2, ksw_align2, ksw_global2) -- TEST INFRASTRUCTURE ONLY.

Written from SURVEY.md Appendix B, in int64; nothing here is shared with oracle/ or with the kernels, and this module imports neither.

What kind of reference each one is:
  * local() and global_() are textbook full-matrix DP: every matrix held whole, a cell's inputs read from the matrices, the band of the
    global alignment a mask.
  * extend() is NOT that.  It is a second restatement of Appendix B's pseudo-code of ksw_extend2, eh[] row included: `_ext_rows` takes every
    input of the recurrence from `found_h` / `found_e`, one reused row, and the band is the beg / end extent that Appendix B trims from row to
    row.  H, E and F are kept whole but only written (apart from the boundary row and column); they serve the comparison of the two row
    forms.  A mask-and-matrix version was written first and disagreed with the oracle and the kernels for reasons that are upstream's
    behaviour, not errors of theirs (oracle/README.md, "What the DP reference found"): untrimmed, an insertion runs right without limit and
    reaches the end of the query where upstream never looks; and an extent that has shrunk and grows again by two columns reads what an
    older row left in eh[].  What the extension reference is independent in: written by another hand in another language from the prose,
    plain int64 with no packed fields, no lanes, no score table, no 2-bit target.
  * Each operation has a vectorised row and a plain-loop twin (`*_scalar`), compared by tests/test_dp_reference.py.  For local and global
    the twin is the whole operation.  For the extension the trim, the tie rules, the gscore rule and the z-drop live in the shared
    `_ext_rows`: the twin checks the inner row (M, E, F, H of one row) and nothing else.

Conventions, all three operations:
  * sequences are codes 0..3, anything above is N; a pair with an N in it scores -1, equal bases +a, different bases -b;
  * scores = (a, b, o_del, e_del, o_ins, e_ins); a gap of length k costs o + k * e;
  * rows i run over the target, columns j over the query; E is the gap that consumes the target (deletion: o_del, e_del), F the one that
    consumes the query (insertion: o_ins, e_ins);
  * matrices are 1-based with a boundary row and column 0: cell [i][j] aligns t[:i] with q[:j].

What each function pins, and what it does not:
  * extend():  score, qle, tle, max_off, gscore (where positive) and gtle (where gscore is positive).  The ties are upstream's: the row
    maximum sits at its LAST column, the best row is the FIRST that reaches the maximum, the best end-of-query row the LAST.
  * local():   the H matrix of the local alignment; ksw_align2's `score` is its maximum, (te, qe) a cell that holds it, and (tb, qb) a start
    from which the global alignment of the two substrings earns the same score.  ksw_align2's `score2` and `te2` (the second-best hit) are
    upstream heuristics over collapsed row maxima with no textbook definition: they stay pinned to the oracle alone.
  * global_(): the optimal banded score.  Among equally good paths ksw_global2's backtrace prefers one; that order stays pinned to the oracle
    alone -- rescore() only says what a CIGAR earns, which lengths it consumes and how far it strays from the diagonal.
"""
import numpy as np

NEG = -(1 << 40)   # "minus infinity" of the global alignment: below every value the recurrence can produce, far from int64's edge


def _sub(scores, tb, q):
    """scores of target base tb against every query base (int64 vector)"""
    a, b = scores[0], scores[1]
    q = np.asarray(q, dtype=np.int64)
    if tb > 3:
        return np.full(q.size, -1, dtype=np.int64)
    return np.where(q > 3, -1, np.where(q == tb, a, -b)).astype(np.int64)


def _sub1(scores, tb, qb):
    if tb > 3 or qb > 3:
        return -1
    return scores[0] if tb == qb else -scores[1]


def ext_band(qlen, scores, w, end_bonus):
    """the band of an extension: min(w, max_ins, max_del), the longest gap each way that a full-length match could still pay for"""
    a, _, o_del, e_del, o_ins, e_ins = scores
    mx = max(a, 0)
    max_ins = max(int(float(qlen * mx + end_bonus - o_ins) / e_ins + 1.), 1)
    max_del = max(int(float(qlen * mx + end_bonus - o_del) / e_del + 1.), 1)
    return min(w, max_ins, max_del)


# ------------------------------------------------------------------------------------------------------------------------------
# anchored extension (ksw_extend2)
# ------------------------------------------------------------------------------------------------------------------------------
def _ext_boundary(qlen, tlen, scores, h0):
    _, _, o_del, e_del, o_ins, e_ins = scores
    H = np.zeros((tlen + 1, qlen + 1), dtype=np.int64)
    H[0][0] = h0
    for j in range(1, qlen + 1):
        H[0][j] = max(h0 - (o_ins + e_ins), 0) if j == 1 else max(H[0][j - 1] - e_ins, 0)
    for i in range(1, tlen + 1):
        H[i][0] = max(h0 - (o_del + e_del * i), 0)
    return H


def _ext_rows(q, t, scores, w, end_bonus, zdrop, h0, row):
    """the row loop of the extension around `row(H, E, F, i, lo, hi, d, e)`: d and e are what cells [i][lo..hi] find on their diagonal and as their E;
    it fills H[i], E[i], F[i] there and returns the E of the cells below.

    A row's extent: columns beg .. end - 1 (0-based), inside the band, and inside what the row above left alive -- Appendix B's trim: leading
    columns whose incoming diagonal and E are both 0 are dropped, the extent ends one column past the last live one.  Appendix B defines the inputs
    of a cell through eh[j]: what column j finds is what was LAST WRITTEN there, by the row above if that row's extent covered it, and by an
    older row (or the first row's initial values) where an extent that had shrunk inside the band grows again by two columns.  `found_h` and `found_e`
    below are that rule; the matrices themselves are kept whole."""
    qlen, tlen = len(q), len(t)
    e_del, e_ins = scores[3], scores[5]
    w = ext_band(qlen, scores, w, end_bonus)
    H = _ext_boundary(qlen, tlen, scores, h0)
    E = np.zeros_like(H)
    F = np.zeros_like(H)
    found_h = H[0].copy()                        # per 0-based column j: the H its cell finds on the diagonal
    found_e = np.zeros(qlen + 1, dtype=np.int64)
    best, best_i, best_j, max_ie, gscore, max_off = h0, -1, -1, -1, -1, 0
    beg, end = 0, qlen
    for i in range(1, tlen + 1):
        i0 = i - 1
        beg, end = max(beg, i0 - w), min(end, i0 + w + 1, qlen)
        m, mj = 0, -1
        h_in = int(H[i][0]) if beg == 0 else 0   # what the next row's first column finds on its diagonal
        last = h_in
        if beg < end:
            found_e[beg:end] = row(H, E, F, i, beg + 1, end, found_h[beg:end].copy(), found_e[beg:end].copy())
            found_h[beg + 1:end + 1] = H[i][beg + 1:end + 1]
            seg = H[i][beg + 1:end + 1]
            m = int(seg.max())                   # the row maximum, at its last column
            mj = beg + int(seg.size - 1 - np.argmax(seg[::-1]))
            last = int(H[i][end])
        found_h[beg] = h_in
        found_e[end] = 0
        if max(beg, end) == qlen:                # the row reaches the end of the query: the later row wins a tie
            if not gscore > last:
                max_ie = i0
            gscore = max(gscore, last)
        if m == 0:
            break
        if m > best:
            best, best_i, best_j = m, i0, mj
            max_off = max(max_off, abs(mj - i0))
        elif zdrop > 0:
            di, dj = i0 - best_i, mj - best_j
            if di > dj:
                if best - m - (di - dj) * e_del > zdrop:
                    break
            elif best - m - (dj - di) * e_ins > zdrop:
                break
        alive = beg + np.flatnonzero((found_h[beg:end + 1] != 0) | (found_e[beg:end + 1] != 0))   # the trim
        inside = alive[alive < end]
        nbeg = int(inside[0]) if inside.size else end
        tail = alive[alive >= nbeg]
        jl = int(tail[-1]) if tail.size else nbeg - 1
        beg, end = nbeg, min(jl + 2, qlen)
    return (best, best_j + 1, best_i + 1, max_ie + 1, gscore, max_off), (H, E, F)


def extend_scalar(q, t, scores, w, end_bonus, zdrop, h0, matrices=False):
    """three plain loops: rows, columns, nothing else"""
    _, _, o_del, e_del, o_ins, e_ins = scores

    def row(H, E, F, i, lo, hi, d, e):
        f, below = 0, []
        for j in range(lo, hi + 1):
            dj, ej = int(d[j - lo]), int(e[j - lo])
            M = dj + _sub1(scores, int(t[i - 1]), int(q[j - 1])) if dj else 0   # a dead cell does not restart on the diagonal
            E[i][j], F[i][j] = ej, f
            H[i][j] = max(M, ej, f)
            below.append(max(ej - e_del, M - (o_del + e_del), 0))                # E and F open from the diagonal term and clamp at 0
            f = max(f - e_ins, M - (o_ins + e_ins), 0)
        return below

    r, mats = _ext_rows(q, t, scores, w, end_bonus, zdrop, h0, row)
    return (r, mats) if matrices else r


def extend(q, t, scores, w, end_bonus, zdrop, h0, matrices=False):
    """(score, qle, tle, gtle, gscore, max_off) of the extension of q against t from an anchor worth h0.

    H[i][j] = max(M, E, F) with M = d + s(t_i, q_j) where the diagonal input d > 0 and 0 otherwise; E and F open from M (not from H) and
    clamp at 0.  Row by row (_ext_rows): the end-of-query score, stop on a row of zeros, then the maximum or the z-drop test.  The row is
    vectorised: M and E depend on the row's inputs alone, and F[j] = max(F[j-1] - e, T[j-1]) with T = max(M - oe, 0) and F[lo] = 0 unrolls to
    max_k<j (T[k] + k e) - (j - 1) e, a running maximum."""
    _, _, o_del, e_del, o_ins, e_ins = scores
    qa = np.asarray(q, dtype=np.int64)

    def row(H, E, F, i, lo, hi, d, e):
        M = np.where(d != 0, d + _sub(scores, int(t[i - 1]), qa[lo - 1:hi]), 0)
        k = np.arange(hi - lo + 1, dtype=np.int64)
        T = np.maximum(M - (o_ins + e_ins), 0)
        run = np.maximum.accumulate(T + k * e_ins)
        f = np.zeros(hi - lo + 1, dtype=np.int64)
        f[1:] = run[:-1] - k[:-1] * e_ins
        E[i][lo:hi + 1], F[i][lo:hi + 1] = e, f
        H[i][lo:hi + 1] = np.maximum(np.maximum(M, e), f)
        return np.maximum(np.maximum(e - e_del, M - (o_del + e_del)), 0)

    r, mats = _ext_rows(q, t, scores, w, end_bonus, zdrop, h0, row)
    return (r, mats) if matrices else r


# ------------------------------------------------------------------------------------------------------------------------------
# local alignment (ksw_align2's forward pass)
# ------------------------------------------------------------------------------------------------------------------------------
def local_scalar(q, t, scores):
    """Gotoh local alignment, three loops: H = max(0, diagonal, E, F); E and F open from H"""
    _, _, o_del, e_del, o_ins, e_ins = scores
    qlen, tlen = len(q), len(t)
    H = np.zeros((tlen + 1, qlen + 1), dtype=np.int64)
    E = np.zeros_like(H)
    F = np.zeros_like(H)
    for i in range(1, tlen + 1):
        for j in range(1, qlen + 1):
            E[i][j] = max(int(E[i - 1][j]) - e_del, int(H[i - 1][j]) - (o_del + e_del), 0)
            F[i][j] = max(int(F[i][j - 1]) - e_ins, int(H[i][j - 1]) - (o_ins + e_ins), 0)
            H[i][j] = max(0, int(H[i - 1][j - 1]) + _sub1(scores, int(t[i - 1]), int(q[j - 1])), int(E[i][j]), int(F[i][j]))
    return H


def local(q, t, scores):
    """the H matrix of the local alignment, (tlen + 1) x (qlen + 1); its maximum is the score.

    Vectorised along the row: F[j] = max(F[j-1] - e, H[j-1] - oe) and H[j-1] = max(G[j-1], F[j-1]) with G = max(0, diagonal, E); as
    F[j-1] - oe <= F[j-1] - e, F[j] = max(F[j-1] - e, G[j-1] - oe): a running maximum of G[k] - oe + k e."""
    _, _, o_del, e_del, o_ins, e_ins = scores
    assert o_ins >= 0 and o_del >= 0
    qa = np.asarray(q, dtype=np.int64)
    qlen, tlen = len(q), len(t)
    H = np.zeros((tlen + 1, qlen + 1), dtype=np.int64)
    E = np.zeros(qlen + 1, dtype=np.int64)
    col = np.arange(qlen + 1, dtype=np.int64)
    for i in range(1, tlen + 1):
        E = np.maximum(np.maximum(E - e_del, H[i - 1] - (o_del + e_del)), 0)
        G = np.zeros(qlen + 1, dtype=np.int64)
        G[1:] = np.maximum(np.maximum(H[i - 1][:-1] + _sub(scores, int(t[i - 1]), qa), E[1:]), 0)
        run = np.maximum.accumulate(G - (o_ins + e_ins) + col * e_ins)
        F = np.zeros(qlen + 1, dtype=np.int64)
        F[1:] = np.maximum(run[:-1] - col[:-1] * e_ins, 0)
        F[1] = 0                                    # nothing to the left of the first column opens a gap
        H[i] = np.maximum(G, F)
        H[i][0] = 0
    return H


# ------------------------------------------------------------------------------------------------------------------------------
# banded global alignment (ksw_global2)
# ------------------------------------------------------------------------------------------------------------------------------
def _glb_boundary(qlen, tlen, scores, w):
    _, _, o_del, e_del, o_ins, e_ins = scores
    H = np.full((tlen + 1, qlen + 1), NEG, dtype=np.int64)
    H[0][0] = 0
    for j in range(1, min(qlen, w) + 1):
        H[0][j] = -(o_ins + e_ins * j)
    for i in range(1, min(tlen, w) + 1):
        H[i][0] = -(o_del + e_del * i)
    return H


def global_scalar(q, t, scores, w):
    """banded global alignment with affine gaps that open from a diagonal step only (a deletion never follows an insertion directly,
    nor the other way round): three loops.  Returns the score of [tlen][qlen] (NEG where the band does not reach it)."""
    _, _, o_del, e_del, o_ins, e_ins = scores
    qlen, tlen = len(q), len(t)
    H = _glb_boundary(qlen, tlen, scores, w)
    M = np.full_like(H, NEG)
    E = np.full_like(H, NEG)
    F = np.full_like(H, NEG)
    for i in range(1, tlen + 1):
        for j in range(1, qlen + 1):
            if abs(i - j) > w:
                continue
            M[i][j] = max(int(H[i - 1][j - 1]) + _sub1(scores, int(t[i - 1]), int(q[j - 1])), NEG)
            E[i][j] = max(int(E[i - 1][j]) - e_del, int(M[i - 1][j]) - (o_del + e_del), NEG)
            F[i][j] = max(int(F[i][j - 1]) - e_ins, int(M[i][j - 1]) - (o_ins + e_ins), NEG)
            H[i][j] = max(int(M[i][j]), int(E[i][j]), int(F[i][j]))
    return int(H[tlen][qlen])


def global_(q, t, scores, w):
    """the optimal score of the global alignment of q and t inside the band |i - j| <= w, gaps opening from a diagonal step only.
    Vectorised along the row like extend(): F is a running maximum of M[k] - oe + k e."""
    _, _, o_del, e_del, o_ins, e_ins = scores
    qa = np.asarray(q, dtype=np.int64)
    qlen, tlen = len(q), len(t)
    H = _glb_boundary(qlen, tlen, scores, w)
    col = np.arange(qlen + 1, dtype=np.int64)
    Mu = np.full(qlen + 1, NEG, dtype=np.int64)
    E = np.full(qlen + 1, NEG, dtype=np.int64)
    for i in range(1, tlen + 1):
        band = np.abs(i - col) <= w
        band[0] = False
        M = np.full(qlen + 1, NEG, dtype=np.int64)
        M[1:] = np.maximum(H[i - 1][:-1] + _sub(scores, int(t[i - 1]), qa), NEG)
        M = np.where(band, M, NEG)
        E = np.where(band, np.maximum(np.maximum(E - e_del, Mu - (o_del + e_del)), NEG), NEG)
        run = np.maximum.accumulate(M - (o_ins + e_ins) + col * e_ins)
        F = np.full(qlen + 1, NEG, dtype=np.int64)
        F[1:] = np.maximum(run[:-1] - col[:-1] * e_ins, NEG)
        F = np.where(band, F, NEG)
        h = np.maximum(np.maximum(M, E), F)
        H[i][1:] = np.where(band[1:], h[1:], NEG)
        Mu = M
    return int(H[tlen][qlen])


def rescore(cigar, q, t, scores):
    """(score, query bases consumed, target bases consumed, largest |i - j| on the way) of a CIGAR given as (op, length) pairs or as BAM words
    (length << 4 | op; 0 = M, 1 = I, 2 = D), walked from the start of both sequences"""
    _, _, o_del, e_del, o_ins, e_ins = scores
    sc = i = j = off = 0
    for c in cigar:
        op, n = (int(c) & 0xf, int(c) >> 4) if np.isscalar(c) or isinstance(c, np.generic) else (int(c[0]), int(c[1]))
        assert n > 0 and op in (0, 1, 2), (op, n)
        if op == 0:
            for k in range(n):
                sc += _sub1(scores, int(t[i + k]), int(q[j + k])) if i + k < len(t) and j + k < len(q) else 0
            i += n
            j += n
        elif op == 1:
            sc -= o_ins + e_ins * n
            j += n
        else:
            sc -= o_del + e_del * n
            i += n
        off = max(off, abs(i - j))
    return sc, j, i, off
