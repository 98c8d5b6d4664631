"""`sambamba markdup' (cmd_markdup, host/sambamba_main.cpp): the output file block by block and record by record against tests/markdup_reference.py, with and
without -r, at every level, with batches that end inside groups, every refusal by its exit code and its one line, and the duplicate names against the project's
own samblaster where the two rules coincide.  CPU-side on the host emulation of the kernels; `-m gpu' on the MI355X."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import markdup_reference as model
import sbl_reference
import view_reference as ref
from common import ROOT
from test_bam_scan import EOF_MARKER, OURS, make_member, reblock
from test_markdup import M, S, P1, P2, mk, random_pairs

SAMTOOLS = os.path.join(ROOT, "oracle", "_ref", "samtools")
CONTIGS = [("mA", 80000), ("mB", 60000)]
READ_GROUPS = [("A", "lib1"), ("B", "lib2"), ("C", "lib1"), ("D", None)]
KNOBS = ("SSG_MARKDUP_BATCH", "SSG_PROF", "SSG_BAM_LEVEL", "SSG_BGZF_DEVICE_LEVELS")


def header(read_groups=READ_GROUPS):
    text = "@HD\tVN:1.3\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CONTIGS)
    text += "".join("@RG\tID:%s\tSM:s%s\n" % (g, "\tLB:" + lb if lb else "") for g, lb in read_groups)
    text = text.encode()
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(CONTIGS))
    for name, ln in CONTIGS:
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    return out


def bam(records, read_groups=READ_GROUPS, per_member=57):
    """a BAM file of these records: the header in a member of its own, every member begins at a record"""
    out = make_member(header(read_groups), "dynamic")
    for i in range(0, len(records), per_member):
        out += make_member(b"".join(records[i:i + per_member]), "dynamic")
    return out + EOF_MARKER


def blocks(data):
    """the payloads of a BGZF file's members, every one inflated by zlib and checked against its CRC and ISIZE"""
    out, o = [], 0
    while o < len(data):
        assert data[o:o + 4] == b"\x1f\x8b\x08\x04" and data[o + 12:o + 14] == b"BC"
        bsize = struct.unpack_from("<H", data, o + 16)[0] + 1
        p = zlib.decompress(data[o + 18:o + bsize - 8], -15)
        assert struct.unpack_from("<II", data, o + bsize - 8) == (zlib.crc32(p), len(p))
        out.append(p)
        o += bsize
    return out


class MarkdupFile:
    """a BAM of seeded templates in generation order, and every run of `markdup' on it"""

    def __init__(self, sambamba, d):
        self.sambamba, self.d, self.runs = sambamba, str(d), {}
        self.clean = {k: v for k, v in os.environ.items() if k not in OURS + KNOBS}
        records = random_pairs(5, 3000)
        # read groups A, B, C of test_markdup's generator, D on a few records: an @RG without LB is library 0, as the records without RG
        self.records = [r if k % 11 else mk(b"d%d" % k, 0, k % 2, 4000 + k % 3, rg=b"D") for k, r in enumerate(records)]
        self.hdr = header()
        open(self.d + "/in.bam", "wb").write(bam(self.records))
        open(self.d + "/skew.bam", "wb").write(reblock(bam(self.records), step=3001))
        self.stream = ref.records(b"".join(self.records), 0)
        self.dup, self.counts = model.compute(self.stream, [g for g, _ in READ_GROUPS], [1, 2, 1, 0])

    def run(self, args, extra=None, out="out.bam"):
        key = (tuple(args), tuple(sorted((extra or {}).items())))
        if key not in self.runs:
            env = dict(self.clean)
            env.update(extra or {})
            if os.path.exists(self.d + "/" + out):
                os.unlink(self.d + "/" + out)
            r = subprocess.run([self.sambamba, "markdup"] + [self.d + "/" + a if a.endswith(".bam") and "/" not in a else a for a in args], capture_output=True, env=env)
            r.stderr = r.stderr.decode()
            r.data = open(self.d + "/" + out, "rb").read() if os.path.exists(self.d + "/" + out) else None
            self.runs[key] = r
        return self.runs[key]

    def records_of(self, r):
        """the run's file: a BGZF file that ends in the marker, the input's header, every block begins at a record; its records' bytes"""
        assert r.returncode == 0 and r.data is not None, r.stderr[-2000:]
        assert r.data.endswith(EOF_MARKER)
        bl = blocks(r.data)
        assert bl[-1] == b"" and all(bl[:-1])
        plain = b"".join(bl)
        assert plain[:len(self.hdr)] == self.hdr
        recs = ref.records(plain, len(self.hdr))
        starts, at = {len(self.hdr)} | {x["off"] for x in recs}, 0
        for p in bl[:-1]:
            assert at == 0 or at in starts, at
            at += len(p)
        return [x["bytes"] for x in recs]


@pytest.fixture(scope="module")
def emu_md(tmp_path_factory, emu_lib):
    return MarkdupFile(os.path.join(ROOT, "tests", "emu", "sambamba_emu"), tmp_path_factory.mktemp("markdup_emu"))


@pytest.fixture(scope="module")
def gpu_md(tmp_path_factory, gpu_lib):
    return MarkdupFile(os.path.join(ROOT, "bin", "sambamba"), tmp_path_factory.mktemp("markdup_gpu"))


def check_output(v):
    assert len(v.dup) > 200 and v.counts["dup_paired"] > 100 and v.counts["dup_fragments"] > 20
    marked, removed = model.expected_bytes(v.stream, v.dup), model.expected_bytes(v.stream, v.dup, remove=True)
    r = v.run(["in.bam", "out.bam"])
    assert v.records_of(r) == marked
    c = v.counts
    line = "[sambamba] markdup: %d records, %d taking part, %d pairs, %d unmatched paired, %d fragments, %d duplicates found" % (
        c["records"], c["taking_part"], c["pairs"], c["unmatched"], c["fragments"], c["dup_paired"] + c["dup_fragments"])
    assert r.stderr.count("\n") == 1 and r.stderr.startswith(line), r.stderr
    if os.path.exists(SAMTOOLS):
        n = subprocess.run([SAMTOOLS, "view", "-c", "-f", "1024", v.d + "/out.bam"], capture_output=True, check=True).stdout
        assert int(n) == sum(1 for b in marked if struct.unpack_from("<H", b, 18)[0] & 0x400)
    assert v.records_of(v.run(["-r", "in.bam", "out.bam"])) == removed
    # the levels; upstream's knobs, taken and ignored
    for args in (["-l", "0"], ["-l", "1", "-t", "2", "-p", "--tmpdir=/nowhere", "--hash-table-size=5", "--overflow-list-size=6", "--sort-buffer-size=7", "--io-buffer-size=8"]):
        assert v.records_of(v.run(args + ["in.bam", "out.bam"])) == marked, args
    # batches that end inside groups and between mates
    for args in ([], ["-r", "-l", "0"]):
        assert v.records_of(v.run(args + ["in.bam", "out.bam"], {"SSG_MARKDUP_BATCH": "20000"})) == (removed if "-r" in args else marked), args
    if "emu" not in v.sambamba:
        r = v.run(["in.bam", "out.bam"], {"SSG_PROF": "1"})
        assert r.returncode == 0 and all("kernel ssg_k_md_%s" % k in r.stderr for k in ("ends", "score", "join", "heads", "mark", "apply")), r.stderr


def test_emu_markdup_command(emu_md):
    check_output(emu_md)


@pytest.mark.gpu
def test_gpu_markdup_command(gpu_md):
    check_output(gpu_md)


def check_command_refusals(v):
    for args, words in ((["in.bam", "in.bam", "out.bam"], "sambamba merge"), (["in.bam"], "usage: sambamba markdup"), (["--frobnicate", "in.bam", "out.bam"], "unsupported option --frobnicate"),
                        (["skew.bam", "out.bam"], "skew.bam is ")):
        r = v.run(args)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.count("\n") == 1 and r.stderr.startswith("[sambamba] ") and words in r.stderr, (args, r.stderr)
        assert r.data is None and not os.path.exists(v.d + "/out.bam")
    with open(v.d + "/in.bam", "rb") as f:
        r = subprocess.run([v.sambamba, "markdup", "/dev/stdin", v.d + "/out.bam"], input=f.read(), capture_output=True, env=v.clean)
    assert r.returncode == 1 and b"not a regular file" in r.stderr and r.stderr.count(b"\n") == 1 and r.stderr.startswith(b"[sambamba] ") and not os.path.exists(v.d + "/out.bam")


def test_emu_markdup_command_refusals(emu_md):
    check_command_refusals(emu_md)


@pytest.mark.gpu
def test_gpu_markdup_command_refusals(gpu_md):
    check_command_refusals(gpu_md)


# ---- the project's own samblaster: where the two rules coincide, the same names are flagged ----
def common_ground(seed, n_pairs):
    """complete pairs, both mates mapped on one contig, no secondary or supplementary lines, one quality everywhere (every score ties: the first seen wins), name
    by name; as (SAM text, BAM records).  Excluded beyond that: CIGARs of clips only and unclipped coordinates below 1 (the reference of samblaster refuses the
    first; nothing here comes near the second)."""
    rng = np.random.RandomState(seed)
    sites = [int(rng.randint(500, 70000)) for _ in range(30)]
    sam, records = ["@HD\tVN:1.3\tSO:unsorted\n"] + ["@SQ\tSN:%s\tLN:%d\n" % c for c in CONTIGS], []
    for k in range(n_pairs):
        tid = int(rng.randint(2))
        ends = []
        for e in range(2):
            clip, rev = int(rng.choice([0, 0, 4, 9])), int(rng.randint(2))
            cig = [(50, M)] if not clip else ([(50 - clip, M), (clip, S)] if rng.randint(2) else [(clip, S), (50 - clip, M)])
            ends.append((sites[rng.randint(len(sites))] + (clip if cig[0][1] == S else 0), rev, cig))
        for e, (pos, rev, cig) in enumerate(ends):
            flag = 0x1 | 0x2 | (0x40, 0x80)[e] | (0x10 if rev else 0) | (0x20 if ends[1 - e][1] else 0)
            records.append(mk(b"c%d" % k, flag, tid, pos, cig, (30,) * 50))
            sam.append("c%d\t%d\t%s\t%d\t30\t%s\t=\t%d\t0\t%s\t%s\n" % (k, flag, CONTIGS[tid][0], pos + 1, "".join("%d%s" % (n, "MIDNSHP=X"[op]) for n, op in cig), ends[1 - e][0] + 1, "A" * 50, "?" * 50))
    return "".join(sam), records


def flagged_names(sam_text):
    return {l.split("\t")[0] for l in sam_text.splitlines() if not l.startswith("@") and int(l.split("\t")[1]) & 0x400}


def check_against_samblaster(sambamba, samblaster, d):
    sam, records = common_ground(17, 2500)
    # the two models agree on this input
    lines = [l.split("\t") for l in sam.splitlines() if not l.startswith("@")]
    blocks_ = [[sbl_reference.Line([c[0] for c in CONTIGS].index(l[2]), int(l[3]), int(l[1]), int(l[4]), l[5]) for l in lines[i:i + 2]] for i in range(0, len(lines), 2)]
    sbl_dup = {lines[2 * i][0] for i, dflag in enumerate(sbl_reference.mark_duplicates(blocks_)) if dflag}
    stream = ref.records(b"".join(records), 0)
    md_dup, _ = model.compute(stream)
    assert {stream[o]["name"].decode() for o in md_dup} == sbl_dup and len(sbl_dup) > 300 and len(md_dup) == 2 * len(sbl_dup)
    # and so do the two programs
    env = {k: v for k, v in os.environ.items() if k not in OURS + KNOBS}
    r = subprocess.run([samblaster], input=sam.encode(), capture_output=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    open(d + "/cg.bam", "wb").write(bam(records, ()))
    r2 = subprocess.run([sambamba, "markdup", d + "/cg.bam", d + "/cg.out.bam"], capture_output=True, env=env)
    assert r2.returncode == 0, r2.stderr[-2000:]
    plain = b"".join(blocks(open(d + "/cg.out.bam", "rb").read()))
    ours = {x["name"].decode() for x in ref.records(plain, len(header(()))) if x["flag"] & 0x400}
    assert ours == flagged_names(r.stdout.decode()) == sbl_dup


def test_emu_markdup_agrees_with_samblaster(tmp_path, emu_lib):
    check_against_samblaster(os.path.join(ROOT, "tests", "emu", "sambamba_emu"), os.path.join(ROOT, "tests", "emu", "samblaster_emu"), str(tmp_path))


@pytest.mark.gpu
def test_gpu_markdup_agrees_with_samblaster(tmp_path, gpu_lib):
    check_against_samblaster(os.path.join(ROOT, "bin", "sambamba"), os.path.join(ROOT, "bin", "samblaster"), str(tmp_path))
