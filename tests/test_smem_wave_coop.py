"""The wave-per-read seeding kernel's chains (csrc/k_smem2.h): the extension whose rank work 16 lanes share, and the chain starts taken from the table of
short-pattern intervals.  Each group has a case on the host emulation and one on the MI355X (`-m gpu`).

  * s2_extend_coop against ssg_bwt_extend1_lean, through ssg_dbg_extend_coop, which runs both on the same (interval, base, direction): all output words equal.
    The two are functions of the numbers they are given, so the constructed inputs need not be intervals of a pattern: they are laid out so that both rank
    queries fall into one block or into two, at positions 1, 64, 65 and 128 of a block, with k == -1, around the primary row, for all four bases and both
    directions -- and the test works out from the inputs, with the formulas of the kernels' comment, that every one of these occurred.  A result of zero
    occurrences comes from the walks: simulated reads (and copies of them with mismatches) extended base by base to the right and to the left, each step's lean
    result the next step's input, a few thousand intervals.  The forward walks are pinned to tests/seed_reference.py as well (the interval of every 7th prefix).
    s2_extend_coop4, the four-at-once form of the kernel's short backward rows, gets every item's interval with its three neighbours', each against the lean form.
    (The wave kernel's backward rows of every length, these among them, are in the table cases below and in tests/test_seed_reference.py's kernel forms.)
  * table starts: every read through the wave kernel (SSG_SMEM_MAX_EXT=1) with tables of K = 0, 2 and 11, and -k 10 under K = 9, 10 and 11 (the cap
    min(K, min_seed_len - 1) of ssg_seed.cpp); the reads of tests/test_seed_reference.py plus reads with an ambiguous base inside the first bases of a start, shorter
    than the table's patterns, shorter than a seed, and with a start two and three bases from the read's end.  The lists must equal those of tests/seed_reference.py
    as multisets (the stage sorts them afterwards) and the extension count must be upstream's: the oracle's bwt_extend calls in mem_collect_intv on the same reads
    (oracle/orc_index.c counts them; tests/test_seed_reference.py pins the oracle's lists to the same reference).
  * resume: budgets under which the lane kernel gives reads up in a later call of pass 1, in pass 2 and inside the third pass; the wave kernel takes each up where
    the lane kernel's record says its unfinished call began (or from the start, when the third pass was unfinished).  ssg_dbg_smem_ext counts the reads by path;
    the lists and the extension count must be the reference's, and over the cases each of the three paths must have run for at least one read.
"""
import ctypes as C

import numpy as np
import pytest

import common
import seed_reference as R
from speedseq_amd import capi

CAP = 128
K10 = (10, 1.5, 10, 500, 20)


# ---------------------------------------------------------------- shared texts, reads and reference results (made once, never changed)
@pytest.fixture(scope="module")
def planted(oracle, tmp_path_factory):
    return common.planted_reference(oracle, tmp_path_factory.mktemp("planted_coop"))


def _text(which, planted):
    return (common.EXAMPLE_FA, None) if which == "golden" else planted


_READS, _WANT = {}, {}


def _reads(prefix, meta):
    if prefix not in _READS:
        sref = common.seed_ref(prefix)
        reads = [r for r in common.fixed_seed_reads(sref, seed=3, planted=meta, n_sim=24, fasta=prefix) if not r[0].startswith("many")]
        base = dict(reads)["exact"]
        for n in (2, 5, 9, 10, 11, 12):                              # shorter than the table's patterns (and than a seed)
            reads.append(("short%d" % n, base[:n].copy()))
        for at in (1, 5, 9, 10, 11):                                 # an ambiguous base inside the first bases of the start at 0 -- and of the start behind it
            q = base.copy(); q[at] = 4; reads.append(("N_at%d" % at, q))
        q = base.copy(); q[40] = 4; q[46] = 4; q[48] = 4; reads.append(("N_40_46_48", q))
        for back in (2, 3, 4, 12):                                   # a start fewer than kt_k bases from the read's end
            q = base.copy(); q[150 - back - 1] = 4; reads.append(("start_%d_from_end" % back, q))
        _READS[prefix] = reads
    return _READS[prefix]


def _want(oracle, prefix, meta, sopt):
    """(reference lists of every read, upstream's bwt_extend count over the reads) once per (text, option set)"""
    if (prefix, sopt) not in _WANT:
        seqs, _, _ = common.cat_reads(_reads(prefix, meta))
        _, oopt, ropt = common.seed_opts(None, oracle, sopt)
        lists = common.seed_reference_lists(common.seed_ref(prefix), seqs, ropt)
        oidx = oracle.idx_load(prefix)
        tot = C.c_uint64.in_dll(oracle.l, "orc_tot_extend")
        n_ext = 0
        for q, w in zip(seqs, lists):
            oracle.l.orc_cnt_flush()
            before = tot.value
            o = oracle.collect_intv(oidx, q, cap=1 << 14, opt=oopt)
            oracle.l.orc_cnt_flush()
            assert len(o) == len(w[0])
            if len(q) >= ropt.min_seed_len:                           # (upstream mem_chain returns before mem_collect_intv on a read shorter than a seed)
                n_ext += tot.value - before
        _WANT[prefix, sopt] = (lists, n_ext)
    return _WANT[prefix, sopt]


# ---------------------------------------------------------------- the shared-rank extension
def _header(prefix):
    w = np.fromfile(prefix + ".sa", dtype=np.uint64, count=7)
    return int(w[0]), [0] + [int(x) for x in w[1:5]], int(w[6])   # primary, L2[0 .. 4], text length


def _classify(x0, x1, x2, back, primary):
    """what ssg_bwt_extend1_lean's comment says of its two rank queries: (k == -1, same block, position of k in its block, of l, holds the primary row, ends on it)"""
    kx = x0 if back else x1
    k, l = kx - 1, kx - 1 + x2
    k2 = 0 if k < 0 else k - (k >= primary)
    l2 = 0 if l < 0 else l - (l >= primary)
    return k < 0, (k2 >> 7) == (l2 >> 7), (k2 & 127) + 1, (l2 & 127) + 1, x2 > 0 and kx <= primary <= kx + x2 - 1, x2 > 0 and kx + x2 - 1 == primary


def _constructed(primary, seq_len):
    """(x0, x1, x2, base, is_back) rows: both queries at every pair of the positions 1, 64, 65, 128 in one block and in two, below, around and above the primary row"""
    rows = []
    n_blk = seq_len >> 7
    pb = primary >> 7
    unrow = lambda r2: r2 if r2 < primary else r2 + 1              # the row whose stored position is r2
    for b1, b2 in ((3, 3), (3, 4), (3, n_blk - 2), (pb, pb), (pb - 1, pb + 1), (pb + 2, pb + 2), (n_blk - 2, n_blk - 2), (0, 0), (0, 1)):
        for a in (0, 63, 64, 127):
            for b in (0, 63, 64, 127):
                k2, l2 = 128 * b1 + a, 128 * b2 + b
                if k2 > l2:
                    continue
                k, l = unrow(k2), unrow(l2)
                for c in range(4):
                    for back in (0, 1):
                        other = (k2 * 7 + 13) % (seq_len + 1 - (l - k)) + 1     # (the other side's numbers are free; the entry wants them inside the text too)
                        rows.append((k + 1, other, l - k, c, back) if back else (other, k + 1, l - k, c, back))
    for x2 in (1, 2, 64, 65, 128, 129, 1000, primary, primary + 1, seq_len + 1):    # k == -1
        for c in range(4):
            for back in (0, 1):
                rows.append((0, 0, x2, c, back))
    for lo in (0, 1, 2, 127, 128, 129):                             # around the primary row: it is the interval's first row, its last, inside, just outside
        for hi in (0, 1, 2, 127, 128):
            for c in range(4):
                for back in (0, 1):
                    kx, x2 = primary - lo, lo + hi
                    rows.append((kx, 9, x2, c, back) if back else (9, kx, x2, c, back))
                    rows.append((primary + 1, 9, hi, c, back) if back else (9, primary + 1, hi, c, back))
    ok = lambda x0, x1, x2, c, back: min(x0, x1, x2) >= 0 and max(x0, x1) + x2 <= seq_len + 1
    assert all(ok(*r) for r in rows), [r for r in rows if not ok(*r)][:3]     # (the texts of these tests are large enough for every row)
    return rows


def _walks(lib, idx, prefix, L2):
    """simulated reads, and copies with a mismatch every 31 bases, extended base by base to the right from their first base and to the left from their last: every
    step's input interval with its base and direction.  Returns (rows, {(read, j): forward interval of the first j bases})"""
    _, seqs, _, _ = common.sim_reads(10, 5, 150, fasta=prefix)
    reads = [s for s in seqs if s.max() < 4][:16]
    reads += [np.where(np.arange(s.size) % 31 == 30, (s + 1) % 4, s).astype(np.uint8) for s in reads[:8]]
    start = lambda c: (L2[c] + 1, L2[3 - c] + 1, L2[c + 1] - L2[c])
    rows, pinned = [], {}
    for back in (0, 1):
        cur = [start(int(q[-1] if back else q[0])) for q in reads]
        for j in range(1, 150):
            base = [int(q[-1 - j]) if back else 3 - int(q[j]) for q in reads]
            iv = np.zeros(len(reads), dtype=capi.INTV_DT)
            iv["x0"], iv["x1"], iv["x2"] = [c[0] for c in cur], [c[1] for c in cur], [c[2] for c in cur]
            rows += [(c[0], c[1], c[2], b, back) for c, b in zip(cur, base)]
            lean = lib.dbg_extend_coop(idx, iv, base, [back] * len(reads))[0]
            cur = [(int(r["x0"]), int(r["x1"]), int(r["x2"])) for r in lean]
            if not back and j % 7 == 0:
                for i in range(len(reads)):
                    pinned[i, j + 1] = cur[i]
    return rows, pinned, reads


def _coop_against_lean(lib, prefix):
    primary, L2, seq_len = _header(prefix)
    idx = lib.index_load(prefix)
    rows = _constructed(primary, seq_len)
    walked, pinned, reads = _walks(lib, idx, prefix, L2)
    sref = common.seed_ref(prefix)
    n_pinned = 0
    for (i, j), got in pinned.items():                                    # the walk itself against the plain-text reference: the first j bases of read i
        want = sref.interval(reads[i], 0, j)
        assert got[2] == want[2] and (want[2] == 0 or got == want[:3]), ("forward walk", i, j, got, want)
        n_pinned += want[2] > 0
    assert n_pinned > 100 and len(walked) > 5000
    rows = rows + walked
    iv = np.zeros(len(rows), dtype=capi.INTV_DT)
    a = np.array(rows, dtype=np.uint64)
    iv["x0"], iv["x1"], iv["x2"] = a[:, 0], a[:, 1], a[:, 2]
    lean, coop, lean4, coop4 = lib.dbg_extend_coop(idx, iv, a[:, 3].astype(np.uint8), a[:, 4].astype(np.uint8))
    lib.index_destroy(idx)
    bad = [t for t in range(len(rows)) if lean[t] != coop[t]]
    assert not bad, ("s2_extend_coop differs from ssg_bwt_extend1_lean", len(bad), rows[bad[0]], lean[bad[0]], coop[bad[0]])
    # four intervals at once: item t's base and direction on the intervals of items t .. t + 3; the first of the four is item t itself
    bad = [(t, g) for t in range(len(rows)) for g in range(4) if lean4[t, g] != coop4[t, g]]
    assert not bad, ("s2_extend_coop4 differs from ssg_bwt_extend1_lean", len(bad), bad[0], rows[bad[0][0]], lean4[bad[0]], coop4[bad[0]])
    assert (lean4[:, 0] == lean).all() and len({(int(r["x0"]), int(r["x1"]), int(r["x2"])) for r in lean4[:200].reshape(-1)}) > 100    # (the four rows of lanes had four different jobs)
    seen = set()
    for t, (x0, x1, x2, c, back) in enumerate(rows):
        kneg, same, rk, rl, holds, ends = _classify(x0, x1, x2, back, primary)
        seen.update([("same", same), ("rk", rk), ("rl", rl), ("base", c, back)])
        seen.update(k for k, v in (("kneg", kneg), ("holds", holds), ("ends", ends), ("zero", int(lean[t]["x2"]) == 0 and x2 > 0)) if v)
        if not kneg:
            seen.add(("pos", same, rk, rl))
    want = {("same", True), ("same", False), "kneg", "holds", "ends", "zero"} | {("base", c, b) for c in range(4) for b in (0, 1)}
    want |= {(w, r) for w in ("rk", "rl") for r in (1, 64, 65, 128)}
    want |= {("pos", False, a, b) for a in (1, 64, 65, 128) for b in (1, 64, 65, 128)} | {("pos", True, a, b) for a in (1, 64, 65, 128) for b in (1, 64, 65, 128) if a <= b}
    assert want <= seen, sorted(map(str, want - seen))
    # and the refusals: a query beyond the text, a base that is none
    idx = lib.index_load(prefix)
    one = np.zeros(1, dtype=capi.INTV_DT)
    one["x0"], one["x2"] = seq_len, 3
    with pytest.raises(capi.SsgError, match="ssg_dbg_extend_coop: need x0 \\+ x2 <= text length \\+ 1 and x1 \\+ x2 <= text length \\+ 1: item 0"):
        lib.dbg_extend_coop(idx, one, [0], [1])
    with pytest.raises(capi.SsgError, match="ssg_dbg_extend_coop: bases are codes 0 .. 3: item 0"):
        lib.dbg_extend_coop(idx, one, [4], [0])
    lib.index_destroy(idx)


@pytest.mark.parametrize("which", ["golden", "planted"])
def test_emu_coop_extension_equals_lean(emu_lib, planted, which):
    _coop_against_lean(emu_lib, _text(which, planted)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["golden", "planted"])
def test_gpu_coop_extension_equals_lean(gpu_lib, planted, which):
    _coop_against_lean(gpu_lib, _text(which, planted)[0])


# ---------------------------------------------------------------- table starts
TABLE_CASES = [("0", None), ("2", None), ("11", None), ("9", K10), ("10", K10), ("11", K10)]
TABLE_IDS = ["K0", "K2", "K11", "k10-K9", "k10-K10", "k10-K11"]


def _wave_kernel_all_reads(lib, oracle, monkeypatch, prefix, meta, K, sopt):
    monkeypatch.setenv("SSG_SMEM_MAX_EXT", "1")                       # every read is given up at its second extension: the wave kernel does them all
    monkeypatch.setenv("SSG_KTAB_K", K)                               # (read when the index is loaded)
    reads = _reads(prefix, meta)
    seqs, seq, off = common.cat_reads(reads)
    want, want_nx = _want(oracle, prefix, meta, sopt)
    opt, _, _ = common.seed_opts(lib, None, sopt)
    idx = lib.index_load(prefix)
    intv, cnt, nx, _ = lib.dbg_smem_ext(idx, opt, seq, off, cap=CAP)
    lib.index_destroy(idx)
    n_iv = 0
    for r, (name, _) in enumerate(reads):
        got = sorted((int(t["info"]), int(t["x0"]), int(t["x1"]), int(t["x2"])) for t in intv[r][:cnt[r]])
        ref = sorted((t[3], t[0], t[1], t[2]) for t in want[r][0])
        assert got == ref, ("the wave kernel disagrees with the seeding reference", prefix, K, sopt, name, got, ref)
        n_iv += len(ref)
    assert n_iv > 100 and any(w[1][1] > 0 for w in want) and any(w[1][2] > 0 for w in want)      # intervals of passes 2 and 3 among them
    assert nx == want_nx, ("extension count", nx, "upstream's", want_nx)


@pytest.mark.parametrize("which", ["golden", "planted"])
@pytest.mark.parametrize("case", TABLE_CASES, ids=TABLE_IDS)
def test_emu_table_starts(emu_lib, oracle, planted, monkeypatch, case, which):
    _wave_kernel_all_reads(emu_lib, oracle, monkeypatch, *_text(which, planted), *case)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["golden", "planted"])
@pytest.mark.parametrize("case", TABLE_CASES, ids=TABLE_IDS)
def test_gpu_table_starts(gpu_lib, oracle, planted, monkeypatch, case, which):
    _wave_kernel_all_reads(gpu_lib, oracle, monkeypatch, *_text(which, planted), *case)


def test_reads_of_the_table_cases_hit_their_edges(planted):
    """from the reads alone: what the table cases are there for occurs with K = 11 (and 9, 10)"""
    for prefix, meta in ((common.EXAMPLE_FA, None), planted):
        reads = dict(_reads(prefix, meta))
        assert min(len(q) for q in reads.values()) == 0 and {2, 5, 9, 10, 11, 12, 18} <= {len(q) for q in reads.values()}
        assert all(reads["N_at%d" % at][at] == 4 for at in (1, 5, 9, 10, 11))
        for back in (2, 3, 4, 12):                                    # the start behind the N has `back' bases to the read's end
            q = reads["start_%d_from_end" % back]
            assert q[150 - back - 1] == 4 and (q[150 - back:] < 4).all() and len(q) - (150 - back) == back


# ---------------------------------------------------------------- resume where the lane kernel's unfinished call began
# budgets under which the lane kernel gives reads up in a later call of pass 1, in pass 2 and inside the third pass (chosen on the emulation, where the counters
# of ssg_dbg_smem_ext say which paths ran; the same settings on the GPU): (SSG_SMEM_MAX_EXT, SSG_SMEM_MAX_ROW, option set)
RESUME_CASES = [("150", "32", None), ("300", "4", None), ("600", "18", None), ("1200", "32", None), ("300", "18", K10), ("900", "4", K10)]
RESUME_IDS = ["e150r32", "e300r4", "e600r18", "e1200r32", "k10-e300r18", "k10-e900r4"]
_PATHS = {}


def _resume(lib, oracle, monkeypatch, prefix, meta, max_ext, max_row, sopt, who):
    monkeypatch.setenv("SSG_SMEM_MAX_EXT", max_ext)
    monkeypatch.setenv("SSG_SMEM_MAX_ROW", max_row)
    reads = _reads(prefix, meta)
    seqs, seq, off = common.cat_reads(reads)
    want, want_nx = _want(oracle, prefix, meta, sopt)
    opt, _, _ = common.seed_opts(lib, None, sopt)
    idx = lib.index_load(prefix)
    intv, cnt, nx, paths = lib.dbg_smem_ext(idx, opt, seq, off, cap=CAP)
    lib.index_destroy(idx)
    for r, (name, _) in enumerate(reads):
        got = sorted((int(t["info"]), int(t["x0"]), int(t["x1"]), int(t["x2"])) for t in intv[r][:cnt[r]])
        ref = sorted((t[3], t[0], t[1], t[2]) for t in want[r][0])
        assert got == ref, ("a resumed read disagrees with the seeding reference", prefix, max_ext, max_row, sopt, name, paths, got, ref)
    assert nx == want_nx, ("extension count", nx, "upstream's", want_nx, paths)
    print("paths", who, prefix.split("/")[-1], max_ext, max_row, sopt, paths)
    tot = _PATHS.setdefault(who, [0, 0, 0, 0])
    for i in range(4):
        tot[i] += paths[i]


@pytest.mark.parametrize("which", ["golden", "planted"])
@pytest.mark.parametrize("case", RESUME_CASES, ids=RESUME_IDS)
def test_emu_resume(emu_lib, oracle, planted, monkeypatch, case, which):
    _resume(emu_lib, oracle, monkeypatch, *_text(which, planted), *case, "emu")


def test_emu_resume_paths_all_ran():
    """over the cases above (this test runs behind them): reads resumed in pass 1 at x > 0, resumed in pass 2, and started again because the third pass was unfinished"""
    assert len(_PATHS.get("emu", [])) == 4 and min(_PATHS["emu"][:3]) > 0, _PATHS


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["golden", "planted"])
@pytest.mark.parametrize("case", RESUME_CASES, ids=RESUME_IDS)
def test_gpu_resume(gpu_lib, oracle, planted, monkeypatch, case, which):
    _resume(gpu_lib, oracle, monkeypatch, *_text(which, planted), *case, "gpu")


@pytest.mark.gpu
def test_gpu_resume_paths_all_ran():
    assert len(_PATHS.get("gpu", [])) == 4 and min(_PATHS["gpu"][:3]) > 0, _PATHS
