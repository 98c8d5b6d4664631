"""BGZF deflate on the device by level (ssg_bgzf_deflate_level, ssg_bgzf_compress_level, ssg_bgzf_compress_recs_level; csrc/k_bgzf_deep.h):
levels 7-9 are a chained match finder in the place of k_bgzf.h's one parse.  Every stream must inflate to its payload (the edges of this kernel among them: a
chunk, a region, a full block, one chain through the whole block, distance 32768 and 32769, matches that run into chunk ends); below level 7 nothing moves;
on a sorted BAM the levels are smaller than the shipped parse; and `sambamba sort' / `merge' pass their level with SSG_BGZF_DEVICE_LEVELS=1 and only then.
CPU-side on the host emulation of the kernel; `-m gpu' on the MI355X, where the streams must also be the emulation's, byte for byte."""
import ctypes as C
import functools
import gzip
import os
import random
import subprocess
import zlib

import numpy as np
import pytest

import simreads
from common import EXAMPLE_FA, ROOT
from speedseq_amd import capi
from test_bam_scan import SHARED, write_sam as write_merge_sam
from test_bgzf_device import bam_like, payloads
from test_sort_device_gather import write_sam

EMU = os.path.join(ROOT, "tests", "emu")
MAXP = 0xff00
SSG_EINVAL = -22


@functools.lru_cache(maxsize=None)
def edges():
    """the payloads at which this kernel takes another path"""
    rng = random.Random(41)
    out = [bam_like(rng, 200)[:n] for n in (0, 1, 3, 4, 5, 63, 64, 65, 4095, 4096, 4097, MAXP)]
    out.append(bytes([7]) * MAXP)                                                   # one chain through the whole block: the depth cap, length 258, distance 1
    x = bytes(rng.getrandbits(8) for _ in range(32769))
    out.append(x[:32768] + x[:32512])                                               # distance exactly 32768 is legal
    out.append(x + x[:32000])                                                       # the only repeats lie at 32769: one of them in the stream and zlib refuses it
    recs = [bytes(rng.getrandbits(8) for _ in range(300)) for _ in range(100)]
    changed = []
    for r in recs:
        k = rng.randrange(300)
        changed.append(r[:k] + bytes([r[k] ^ 0x55]) + r[k + 1:])
    out.append(b"".join(recs) + b"".join(changed))                                  # matches run into chunk ends
    return out


def deflate(lib, blocks, level):
    """the blocks' streams at a level (None: ssg_bgzf_deflate)"""
    cut = np.zeros(len(blocks) + 1, dtype=np.uint64)
    cut[1:] = np.cumsum([len(b) for b in blocks])
    out, off = capi.bgzf_deflate(lib, b"".join(blocks), cut, level)
    return [out[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(blocks))]


def check_inflates(lib, seed, big):
    blocks = payloads(seed, big)
    n_pay = len(blocks)
    blocks = blocks + edges()
    res = {}
    for level in (7, 9):
        streams = res[level] = deflate(lib, blocks, level)
        for i, (b, s) in enumerate(zip(blocks, streams)):
            assert len(s) <= len(b) + 5, (level, i, len(s), len(b))
            d = zlib.decompressobj(-15)
            got = d.decompress(s)
            assert d.eof and d.unused_data == b"", (level, i, len(b))              # one final block, nothing behind it
            assert got == b, (level, i, len(b), len(got))
        i_max, i_run, i_32768, i_32769, i_recs = (n_pay + k for k in (11, 12, 13, 14, 15))
        assert len(streams[i_run]) < 1200                                           # the run is found at every position
        assert len(streams[i_32768]) < 32768 + 4000                                 # the repeat at distance 32768 is used: 508 chunks, a match of at most 5 bytes each
        assert len(streams[i_32769]) == len(blocks[i_32769]) + 5                    # noise without a legal repeat: stored
        assert len(streams[i_recs]) < 30000 + 12000                                 # the second half costs a fraction of the first
    return blocks, res


def test_emu_level_streams_inflate_to_their_payload(emu_lib):
    check_inflates(emu_lib, 5, big=False)


@pytest.mark.gpu
def test_gpu_level_streams_inflate_to_their_payload_and_equal_the_emulation(gpu_lib):
    blocks, res = check_inflates(gpu_lib, 6, big=True)
    for level in (7, 9):
        assert deflate(gpu_lib, blocks, level) == res[level]                        # the parse is deterministic
    so = os.path.join(EMU, "libssgpu_emu.so")
    if os.path.exists(so):
        emu = capi.Lib(so)
        for level in (7, 9):
            theirs = deflate(emu, blocks, level)
            diff = [i for i in range(len(blocks)) if theirs[i] != res[level][i]]
            assert not diff, (level, diff)


def check_below_7(lib):
    blocks = payloads(5, False)
    cut = np.zeros(len(blocks) + 1, dtype=np.uint64)
    cut[1:] = np.cumsum([len(b) for b in blocks])
    pay = b"".join(blocks)
    plain = deflate(lib, blocks, None)
    members, moff, crc = capi.bgzf_compress(lib, pay, cut)
    for level in (1, 6):
        assert deflate(lib, blocks, level) == plain
        m, o, c = capi.bgzf_compress(lib, pay, cut, level=level)
        assert m.tobytes() == members.tobytes() and (o == moff).all() and (c == crc).all()
    m9, o9, c9 = capi.bgzf_compress(lib, pay, cut, level=9)                         # framed, the level's streams: a BGZF file's body
    assert gzip.decompress(m9.tobytes()) == pay and (c9 == crc).all() and int(o9[-1]) < int(moff[-1])
    p = np.frombuffer(pay, dtype=np.uint8)
    out = np.zeros(len(pay) + 31 * len(blocks) + 64, dtype=np.uint8)
    off = np.zeros(len(blocks) + 1, dtype=np.uint64)
    args = (p.ctypes.data_as(C.c_void_p), cut.ctypes.data_as(C.c_void_p), C.c_long(len(blocks)), out.ctypes.data_as(C.c_void_p), C.c_uint64(out.size), off.ctypes.data_as(C.c_void_p))
    for level in (0, 10, -1):
        assert lib.l.ssg_bgzf_deflate_level(*args, C.c_int(level)) == SSG_EINVAL
        assert b"level" in lib.l.ssg_last_error()
        assert lib.l.ssg_bgzf_compress_level(*args, None, C.c_int(level)) == SSG_EINVAL
        assert lib.l.ssg_bgzf_compress_recs_level(None, cut.ctypes.data_as(C.c_void_p), C.c_long(len(blocks)), out.ctypes.data_as(C.c_void_p), C.c_uint64(out.size),
                                                   off.ctypes.data_as(C.c_void_p), None, C.c_int(level)) == SSG_EINVAL


def test_emu_nothing_moves_below_level_7(emu_lib):
    emu_lib.l.ssg_last_error.restype = C.c_char_p
    check_below_7(emu_lib)


@pytest.mark.gpu
def test_gpu_nothing_moves_below_level_7(gpu_lib):
    gpu_lib.l.ssg_last_error.restype = C.c_char_p
    check_below_7(gpu_lib)


@pytest.fixture(scope="module")
def sorted_bam_blocks(tmp_path_factory, emu_lib):
    """the sorted main BAM of 2000 simulated pairs of the bundled slice through the emulation executables (bwa mem | samblaster | sambamba view | sambamba sort),
    inflated and cut at 0xff00"""
    d = str(tmp_path_factory.mktemp("bgzf_levels_bam"))
    fq = d + "/r.fq.gz"
    simreads.write_fastq(fq, simreads.simulate(simreads.read_fasta(EXAMPLE_FA), 2000, seed=23))
    p1 = subprocess.run([os.path.join(EMU, "bwa_emu"), "mem", "-t", "4", "-p", "-R", "@RG\\tID:g\\tSM:s\\tLB:l", EXAMPLE_FA, fq], capture_output=True, check=True, timeout=900)
    p2 = subprocess.run([os.path.join(EMU, "samblaster_emu"), "--addMateTags"], input=p1.stdout, capture_output=True, check=True)
    p3 = subprocess.run([os.path.join(EMU, "sambamba_emu"), "view", "-S", "-f", "bam", "-l", "0", "/dev/stdin"], input=p2.stdout, capture_output=True, check=True)
    with open(d + "/u.bam", "wb") as f:
        f.write(p3.stdout)
    subprocess.run([os.path.join(EMU, "sambamba_emu"), "sort", "-t", "4", "-m", "1G", "--tmpdir=" + d + "/tmp", "-l", "1", "-o", d + "/s.bam", d + "/u.bam"], check=True, capture_output=True)
    raw = gzip.decompress(open(d + "/s.bam", "rb").read())
    blocks = [raw[k:k + MAXP] for k in range(0, len(raw), MAXP)]
    assert len(blocks) >= 8
    return blocks


def check_worth_having(lib, blocks):
    n = sum(len(b) for b in blocks)
    dev = {level: sum(len(s) for s in deflate(lib, blocks, level)) for level in (6, 7, 8, 9)}
    z = {}
    for level in (1, 6, 9):
        z[level] = 0
        for b in blocks:
            o = zlib.compressobj(level, zlib.DEFLATED, -15)
            z[level] += len(o.compress(b) + o.flush())
    print("\n%d blocks, %d bytes: device level 6 %d (%.4f)  7 %d (%.4f)  8 %d (%.4f)  9 %d (%.4f);  zlib 1 %d (%.4f)  6 %d (%.4f)  9 %d (%.4f);  9 %s 7"
          % (len(blocks), n, dev[6], dev[6] / n, dev[7], dev[7] / n, dev[8], dev[8] / n, dev[9], dev[9] / n, z[1], z[1] / n, z[6], z[6] / n, z[9], z[9] / n,
             "beats" if dev[9] < dev[7] else "does not beat"))
    assert dev[7] < dev[6] and dev[9] < dev[6], dev                                  # on the sum, not block by block


def test_emu_levels_are_smaller_on_a_sorted_bam(emu_lib, sorted_bam_blocks):
    check_worth_having(emu_lib, sorted_bam_blocks)


@pytest.mark.gpu
def test_gpu_levels_are_smaller_on_a_sorted_bam(gpu_lib, sorted_bam_blocks):
    check_worth_having(gpu_lib, sorted_bam_blocks)


# ---------------- through the executable ----------------
OURS = ("SSG_BGZF_DEVICE_LEVELS", "SSG_BGZF_DEVICE", "SSG_BAM_LEVEL", "SSG_SORT_DEVICE_GATHER", "SSG_BGZF_DEVICE_CRC", "SSG_SORT_CHUNK_BYTES", "SSG_BGZF_FAIL_AFTER", "SSG_SORT_HOST_BATCHES",
        "SSG_SORT_RUN_DEVICE", "SSG_SORT_DEV_BATCH", "SSG_MERGE_DEVICE", "SSG_MERGE_WINDOW", "SSG_INDEX_DEVICE", "SSG_SORT_NO_BAI", "SSG_DEBUG", "SSG_SORT_LOG")
ON = {"SSG_BGZF_DEVICE_LEVELS": "1"}


class Tool:
    """one unsorted BAM per session and binary; every run of `sambamba sort' on it under another environment and level"""

    def __init__(self, sambamba, d):
        self.sambamba, self.d, self.runs = sambamba, str(d), {}
        self.clean = {k: v for k, v in os.environ.items() if k not in OURS}
        write_sam(self.d + "/in.sam")
        self.view(self.d + "/in.sam", self.d + "/u.bam")

    def view(self, sam, bam):
        with open(sam, "rb") as fi, open(bam, "wb") as fo:
            subprocess.run([self.sambamba, "view", "-S", "-f", "bam", "-l", "0", "/dev/stdin"], stdin=fi, stdout=fo, check=True, env=self.clean)

    def sort(self, tag, extra, args=(), src=None):
        if tag not in self.runs:
            env = dict(self.clean, SSG_BGZF_DEVICE="1", SSG_SORT_LOG="1"); env.update(extra)
            out = "%s/%s.bam" % (self.d, tag)
            r = subprocess.run([self.sambamba, "sort", "-t", "4", "-m", "1G", "--tmpdir=%s/tmp_%s" % (self.d, tag)] + list(args) + ["-o", out, src or self.d + "/u.bam"],
                               check=True, capture_output=True, text=True, env=env)
            self.runs[tag] = (open(out, "rb").read(), open(out + ".bai", "rb").read(), r.stderr, out)
        return self.runs[tag]

    def host_index(self, bam):
        """the .bai the host `sambamba index' writes for a copy of the file (no note of a writer next to it)"""
        tmp = "%s/ix_%d.bam" % (self.d, len(os.listdir(self.d)))
        open(tmp, "wb").write(open(bam, "rb").read())
        subprocess.run([self.sambamba, "index", "-t", "4", tmp], check=True, capture_output=True, env=self.clean)
        return open(tmp + ".bai", "rb").read()


def deflated_line(log):
    line = [l for l in log.split("\n") if "blocks deflated on" in l]
    assert len(line) == 1, log[-1500:]
    return line[0]


def check_sort(t):
    off_bam, off_bai, off_log, _ = t.sort("off_6", {}, ["-l", "6"])
    assert "device deflate level" not in off_log
    on_bam, on_bai, on_log, _ = t.sort("on_6", ON, ["-l", "6"])
    assert on_bam == off_bam and on_bai == off_bai                                  # up to level 6 the switch changes nothing
    assert "device deflate level 6" in deflated_line(on_log) and "k_bgzf.h" in deflated_line(on_log)
    off9_bam, off9_bai, _, _ = t.sort("off_9", {}, ["-l", "9"])                     # without the switch the device has one level
    assert off9_bam == off_bam and off9_bai == off_bai
    for tag, extra, args in (("on_9", ON, ["-l", "9"]), ("env_9", dict(ON, SSG_BAM_LEVEL="9"), [])):
        bam, bai, log, path = t.sort(tag, extra, args)
        assert gzip.decompress(bam) == gzip.decompress(off_bam)                      # every member's CRC-32 and ISIZE hold, the same stream
        assert len(bam) < len(off_bam), (tag, len(bam), len(off_bam))
        assert bai == t.host_index(path)
        assert "device deflate level 9" in deflated_line(log) and "chained match finder" in deflated_line(log), log[-1500:]
    assert t.sort("on_9", ON, ["-l", "9"])[0] == t.sort("env_9", dict(ON, SSG_BAM_LEVEL="9"), [])[0]
    # the device "fails" from its second batch on: the host's pool finishes the file with zlib at that level
    bam, _, log, _ = t.sort("fail_9", dict(ON, SSG_BGZF_FAIL_AFTER="1", SSG_SORT_DEV_BATCH="16"), ["-l", "9"])
    assert "compressing the rest of the output on the host (zlib level 9)" in log and gzip.decompress(bam) == gzip.decompress(off_bam)


@pytest.fixture(scope="module")
def emu_tool(tmp_path_factory, emu_lib):
    return Tool(os.path.join(EMU, "sambamba_emu"), tmp_path_factory.mktemp("bgzf_levels_emu"))


@pytest.fixture(scope="module")
def gpu_tool(tmp_path_factory, gpu_lib):
    return Tool(os.path.join(ROOT, "bin", "sambamba"), tmp_path_factory.mktemp("bgzf_levels_gpu"))


def test_emu_sambamba_sort_passes_its_level_with_the_switch(emu_tool):
    check_sort(emu_tool)


@pytest.mark.gpu
def test_gpu_sambamba_sort_passes_its_level_with_the_switch(gpu_tool):
    check_sort(gpu_tool)


def check_merge(t):
    ins = []
    for name, seed, n, tail, rg in (("ma", 1, 1500, 300, "ga"), ("mb", 2, 1200, 100, "gb")):
        write_merge_sam("%s/%s.sam" % (t.d, name), seed, n, tail, SHARED, rg)
        t.view("%s/%s.sam" % (t.d, name), "%s/%s.u.bam" % (t.d, name))
        ins.append(t.sort(name, {"SSG_BGZF_DEVICE": "0"}, [], src="%s/%s.u.bam" % (t.d, name))[3])
    outs = {}
    for tag, extra, args in (("host", {}, []), ("dev", {"SSG_MERGE_DEVICE": "1"}, []), ("dev_9", dict(ON, SSG_MERGE_DEVICE="1"), ["-l", "9"])):
        out = "%s/merged_%s.bam" % (t.d, tag)
        r = subprocess.run([t.sambamba, "merge", "-t", "4"] + args + [out] + ins, capture_output=True, text=True, env=dict(t.clean, SSG_DEBUG="1", **extra))
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = (open(out, "rb").read(), r.stderr, out)
    line = [l for l in outs["dev_9"][1].split("\n") if "merged on the device" in l]
    assert len(line) == 1 and "device deflate level 9: chained match finder" in line[0], outs["dev_9"][1][-2000:]
    assert "device deflate level" not in outs["dev"][1] and "merged on the device" in outs["dev"][1]
    assert gzip.decompress(outs["dev_9"][0]) == gzip.decompress(outs["host"][0])    # the same records in the same order under the same header
    assert len(outs["dev_9"][0]) < len(outs["dev"][0])
    assert open(outs["dev_9"][2] + ".bai", "rb").read() == t.host_index(outs["dev_9"][2])


def test_emu_sambamba_merge_passes_its_level_with_the_switch(emu_tool):
    check_merge(emu_tool)


@pytest.mark.gpu
def test_gpu_sambamba_merge_passes_its_level_with_the_switch(gpu_tool):
    check_merge(gpu_tool)
