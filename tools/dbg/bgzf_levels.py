#!/usr/bin/env python3
"""Size and time of the device's BGZF deflate by level (csrc/k_bgzf.h: levels 1-6; csrc/k_bgzf_deep.h: levels 7-9); the sibling of bgzf_ratio_emu.py.
usage: bgzf_levels.py emu [--pairs N] [--blocks B] [--levels 6,7,8,9] [--lib LIB] [--out FILE.json]
           ratio per level next to zlib 1 / 6 / 9 on the host emulation of the kernels (CPU), every stream inflated with zlib, on two payloads: the first B
           blocks of the coordinate-sorted BAM of N simulated 2x150 pairs of the bundled slice with binned qualities (the payload of
           profiles/r06_bgzf_ratio_experiments.txt; made here with the emulation executables) and test_bgzf_device.py's bam_like records
       bgzf_levels.py gpu [--blocks 4096] [--repeats 3] [--out FILE.json]
           one ssg_bgzf_compress_level call of BAM-shaped blocks per level on the device, levels alternating, the deflate kernel's device time from ssg_prof_get
With --out the result is merged into the JSON file under the mode's key."""
import argparse
import gzip
import json
import os
import random
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
EMU = os.path.join(ROOT, "tests", "emu")
MAXP = 0xff00


def sorted_bam_payload(n_pairs, seed=7):
    """the inflated stream of the sorted main BAM of n_pairs simulated pairs: bwa mem | samblaster | sambamba view | sambamba sort, all emulation builds.  Qualities
    binned as a recent Illumina instrument writes them: Q37 with a probability falling from 0.85 to 0.55 along the read, else one of Q11 / Q25 / Q37"""
    import simreads
    from common import EXAMPLE_FA
    rng = np.random.default_rng(seed)
    pairs = simreads.simulate(simreads.read_fasta(EXAMPLE_FA), n_pairs, seed=seed)
    with tempfile.TemporaryDirectory() as d:
        fq = os.path.join(d, "r.fq")
        with open(fq, "wb") as f:
            for name, r1, r2 in pairs:
                for e, r in ((1, r1), (2, r2)):
                    p37 = np.linspace(0.85, 0.55, r.size)
                    q = np.where(rng.random(r.size) < p37, 37, rng.choice([11, 25, 37], size=r.size))
                    f.write(b"@" + name.encode() + b"/%d\n" % e + simreads.BASES[r].tobytes() + b"\n+\n" + (q + 33).astype(np.uint8).tobytes() + b"\n")
        p1 = subprocess.run([os.path.join(EMU, "bwa_emu"), "mem", "-t", "8", "-p", "-R", "@RG\\tID:g\\tSM:s\\tLB:l", EXAMPLE_FA, fq], capture_output=True, check=True)
        p2 = subprocess.run([os.path.join(EMU, "samblaster_emu"), "--addMateTags"], input=p1.stdout, capture_output=True, check=True)
        p3 = subprocess.run([os.path.join(EMU, "sambamba_emu"), "view", "-S", "-f", "bam", "-l", "0", "/dev/stdin"], input=p2.stdout, capture_output=True, check=True)
        with open(os.path.join(d, "u.bam"), "wb") as f:
            f.write(p3.stdout)
        subprocess.run([os.path.join(EMU, "sambamba_emu"), "sort", "-t", "4", "-m", "1G", "--tmpdir=" + d, "-l", "1", "-o", os.path.join(d, "s.bam"), os.path.join(d, "u.bam")], check=True, capture_output=True)
        return gzip.decompress(open(os.path.join(d, "s.bam"), "rb").read())


def zlib_raw(b, lvl):
    o = zlib.compressobj(lvl, zlib.DEFLATED, -15)
    return len(o.compress(b) + o.flush())


def sizes(lib, blocks, level):
    """summed stream bytes of the blocks at a level (None: ssg_bgzf_deflate), every stream checked with zlib's inflate"""
    from speedseq_amd import capi
    cut = np.zeros(len(blocks) + 1, dtype=np.uint64)
    cut[1:] = np.cumsum([len(b) for b in blocks])
    out, off = capi.bgzf_deflate(lib, b"".join(blocks), cut, level)
    for i, b in enumerate(blocks):
        d = zlib.decompressobj(-15)
        assert d.decompress(out[int(off[i]):int(off[i + 1])].tobytes()) == b and d.eof, (level, i)
    return int(off[-1])


def mode_emu(a):
    from speedseq_amd import capi
    from test_bgzf_device import bam_like
    lib = capi.Lib(a.lib or os.path.join(EMU, "libssgpu_emu.so"))
    raw = sorted_bam_payload(a.pairs)
    sets = {"sorted_bam": [raw[k:k + MAXP] for k in range(0, len(raw), MAXP)][:a.blocks]}
    d = bam_like(random.Random(5), 1300)
    sets["bam_like"] = [d[k:k + MAXP] for k in range(0, len(d), MAXP)][:a.blocks]
    res = {}
    for name, blocks in sets.items():
        n = sum(len(b) for b in blocks)
        r = {"blocks": len(blocks), "payload_bytes": n}
        for lvl in (1, 6, 9):
            r["zlib_%d" % lvl] = round(sum(zlib_raw(b, lvl) for b in blocks) / n, 4)
        for lvl in a.levels:
            r["device_%d" % lvl] = round(sizes(lib, blocks, lvl) / n, 4)
        res[name] = r
        print(name, json.dumps(r))
    return res


def mode_gpu(a):
    from speedseq_amd import capi
    from test_bgzf_device import bam_like
    lib = capi.Lib(a.lib) if a.lib else capi.Lib()
    lib.l.ssg_prof_enable(1)
    d = bam_like(random.Random(5), 1300)
    base = [d[k:k + MAXP] for k in range(0, len(d) - MAXP, MAXP)]
    blocks = [base[i % len(base)] for i in range(a.blocks)]
    pay = np.frombuffer(b"".join(blocks), dtype=np.uint8)
    cut = np.zeros(len(blocks) + 1, dtype=np.uint64)
    cut[1:] = np.cumsum([len(b) for b in blocks])
    res = {"blocks": len(blocks), "payload_bytes": int(cut[-1]), "levels": {}}
    for lvl in a.levels:
        capi.bgzf_compress(lib, pay, cut, want_crc=False, level=lvl)   # warm-up
    for rep in range(a.repeats):
        for lvl in a.levels:
            lib.l.ssg_prof_reset()
            t0 = time.time()
            out, off, _ = capi.bgzf_compress(lib, pay, cut, want_crc=False, level=lvl)
            wall = time.time() - t0
            prof = {k: v[0] for k, v in capi.prof_get(lib).items() if "deflate" in k}
            e = res["levels"].setdefault(str(lvl), {"member_bytes": int(off[-1]), "ratio": round(int(off[-1]) / int(cut[-1]), 4), "kernel_ms": [], "call_ms": []})
            e["kernel_ms"].append({k: round(v, 3) for k, v in prof.items()})
            e["call_ms"].append(round(wall * 1e3, 1))
    print(json.dumps(res, indent=1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["emu", "gpu"])
    ap.add_argument("--pairs", type=int, default=6000)
    ap.add_argument("--blocks", type=int, default=None)
    ap.add_argument("--levels", default="6,7,8,9")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lib")
    ap.add_argument("--out")
    a = ap.parse_args()
    a.levels = [int(x) for x in a.levels.split(",")]
    if a.blocks is None:
        a.blocks = 8 if a.mode == "emu" else 4096
    res = mode_emu(a) if a.mode == "emu" else mode_gpu(a)
    if a.out:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
        doc[a.mode] = res
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
