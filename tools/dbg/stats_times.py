#!/usr/bin/env python3
"""`sambamba stats' against the reference's samtools 1.3.1 (oracle/_ref/samtools stats) on one box: a coordinate-sorted BAM of N simulated pairs (2x150) made with
the project's own `sambamba view' and `sort'; the whole command against `samtools stats', two alternating runs each after a warm-up, the outputs compared by the
rule of tests/test_stats.py (every line that is neither a comment nor GCD, without trailing comments).  One more device run under SSG_PROF=1 gives the kernels'
times; the per-base kernel's is set against ssg_k_bgzf_inflate's for the same members.  --resources compiles csrc/ssg_stats.cpp once more with the compiler's
resource remarks and records VGPRs, SGPRs, LDS, scratch and occupancy of every kernel (no device needed); a timing run keeps what an earlier --resources run left
in the output file.  Everything goes to profiles/stats_times.json (--out names another place).  A tool, not a test: no ratio is asserted.
usage: stats_times.py [--pairs N] [--threads T] [--out FILE] [--resources] [--sambamba PATH]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OURS = ("SSG_STATS_SPAN", "SSG_STATS_TILE", "SSG_STATS_SLAB", "SSG_PROF", "SSG_DEBUG")
CTG = [("chr%d" % (i + 1), 40000000) for i in range(8)]
SAMTOOLS = os.path.join(ROOT, "oracle", "_ref", "samtools")
DEFAULT_OUT = os.path.join(ROOT, "profiles", "stats_times.json")


def write_sam(path, n, seed=7):
    rng = np.random.RandomState(seed)
    with open(path, "wb") as f:
        f.write(("@HD\tVN:1.3\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CTG)).encode())
        step = 50000
        for a in range(0, n, step):
            m = min(step, n - a)
            seqs = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.choice(5, size=(2 * m, 150), p=[0.245, 0.25, 0.25, 0.245, 0.01])]
            quals = (33 + rng.choice([40, 40, 37, 25, 12, 2], size=(2 * m, 150))).astype(np.uint8)
            ctg = rng.randint(len(CTG), size=m); pos = rng.randint(1, CTG[0][1] - 1000, size=m); ins = rng.randint(200, 600, size=m); nm = rng.randint(0, 5, size=2 * m)
            out = []
            for i in range(m):
                name, c = b"sim_%d" % (a + i), CTG[ctg[i]][0].encode()
                p1, p2 = int(pos[i]), int(pos[i] + ins[i])
                cig = b"150M" if (a + i) % 9 else b"70M2D80M" if (a + i) % 2 else b"60M3I87M"
                out.append(b"%s\t99\t%s\t%d\t60\t%s\t=\t%d\t%d\t%s\t%s\tNM:i:%d\n" % (name, c, p1, cig, p2, p2 - p1 + 150, seqs[2 * i].tobytes(), quals[2 * i].tobytes(), nm[2 * i]))
                out.append(b"%s\t%d\t%s\t%d\t60\t150M\t=\t%d\t%d\t%s\t%s\tNM:i:%d\n" % (name, 147 | (1024 if (a + i) % 50 == 0 else 0), c, p2, p1, p1 - p2 - 150, seqs[2 * i + 1].tobytes(), quals[2 * i + 1].tobytes(), nm[2 * i + 1]))
            f.write(b"".join(out))


def run(cmd, extra, stdout, limit_s=1500):
    env = {k: v for k, v in os.environ.items() if k not in OURS}
    env.update(extra)
    t = time.perf_counter()
    with open(stdout, "wb") as fo:
        r = subprocess.run(cmd, stdout=fo, stderr=subprocess.PIPE, text=True, env=env, timeout=limit_s)
    t = time.perf_counter() - t
    if r.returncode != 0:
        raise SystemExit("%s failed (rc %d): %s" % (" ".join(cmd), r.returncode, r.stderr[-1500:]))
    return round(t, 3), r.stderr.split("\n")


def numbers(path):
    return [l.split("\t# ")[0] for l in open(path).read().splitlines() if not l.startswith("#") and not l.startswith("GCD")]


def kernels(log):
    out = {}
    for l in log:
        m = re.search(r": kernel (\S+)\s+([0-9.]+) ms in (\d+) launches", l)
        if m:
            out[m.group(1)] = {"ms": float(m.group(2)), "launches": int(m.group(3))}
    return out


def resources():
    """the compiler's remarks on the kernels of csrc/ssg_stats.cpp, compiled as the Makefile compiles it"""
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip", "-c", os.path.join(ROOT, "speedseq_amd", "csrc", "ssg_stats.cpp"),
                            "-o", td + "/x.o", "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("hipcc failed: " + r.stderr[-1500:])
    out, cur = {}, None
    keys = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane", "Occupancy [waves/SIMD]": "occupancy_waves_per_simd", "LDS Size [bytes/block]": "lds_bytes"}
    for l in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", l)
        if m:
            k = re.search(r"ssg_k_stats_[a-z_]+?(?=PK|P[a-z]|$)", m.group(1))
            cur = k.group(0) if k else None
            if cur:
                out[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z\[\]/ ]+): (\d+)", l)
        if m and cur and m.group(1) in keys:
            out[cur][keys[m.group(1)]] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2000000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--sambamba", default=os.path.join(ROOT, "bin", "sambamba"), help="another build of the executable (tests/emu/sambamba_emu: the host emulation, to try the tool without a device)")
    a = ap.parse_args()
    kept = {}
    for p in (a.out, DEFAULT_OUT):
        if not kept and os.path.exists(p):
            kept = json.load(open(p))
    if a.resources:
        kept["kernel_resources"] = resources()
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(kept, open(a.out, "w"), indent=1)
        print(json.dumps(kept["kernel_resources"]))
        return 0
    sambamba = a.sambamba
    if not os.path.exists(SAMTOOLS):
        raise SystemExit("%s is not there: __graft_entry__.build() makes it from the reference" % SAMTOOLS)
    td_obj = tempfile.TemporaryDirectory(); td = td_obj.name
    sam, ubam, bam = td + "/in.sam", td + "/in.u.bam", td + "/in.bam"
    t = time.perf_counter()
    write_sam(sam, a.pairs)
    clean = {k: v for k, v in os.environ.items() if k not in OURS}
    with open(sam, "rb") as fi, open(ubam, "wb") as fo:
        subprocess.run([sambamba, "view", "-S", "-f", "bam", "/dev/stdin"], stdin=fi, stdout=fo, check=True, env=clean)
    os.remove(sam)
    subprocess.run([sambamba, "sort", "-t", str(a.threads), "-m", "32G", "--tmpdir=%s/tmp" % td, "-o", bam, ubam], check=True, capture_output=True, env=clean)
    os.remove(ubam)
    print("input made in %.0f s: %d bytes" % (time.perf_counter() - t, os.path.getsize(bam)), flush=True)
    res = {"what": "sambamba stats (device) against samtools 1.3.1 stats (host, one thread) on a coordinate-sorted BAM of %d simulated pairs (2x150, an indel in one read of nine, "
                   "a duplicate per 50 pairs, NM on every record) over 8 contigs of 40 Mb; wall seconds of the whole command with the output written to a file; the first run of "
                   "each warms the page cache and is not kept" % a.pairs,
           "pairs": a.pairs, "threads_of_the_box": os.cpu_count(), "bam_bytes": os.path.getsize(bam)}
    jobs = {"stats": [sambamba, "stats", bam], "samtools_stats": [SAMTOOLS, "stats", bam]}
    for name in jobs:
        res[name + "_s"] = []
    for rep in range(3):
        for name, cmd in jobs.items():
            w, _ = run(cmd, {}, "%s/%s.out" % (td, name))
            if rep:
                res[name + "_s"].append(w)
            print("%s: %.2f s" % (name, w), flush=True)
    ours, theirs = numbers(td + "/stats.out"), numbers(td + "/samtools_stats.out")
    res["lines_compared"] = len(theirs)
    res["stats_equals_samtools_stats"] = ours == theirs
    if ours != theirs:
        res["first_differences"] = [(x, y) for x, y in zip(ours, theirs) if x != y][:5]
    w, log = run(jobs["stats"], {"SSG_PROF": "1"}, td + "/prof.out")                                              # (HIP events around every launch: not a timed run)
    k = kernels(log)
    res["prof"] = {"wall_s": w, "kernels": k}
    if k.get("ssg_k_stats_bases", {}).get("ms", 0) > 0:
        res["bases_per_s_of_the_per_base_kernel"] = round(2 * a.pairs * 150 / (k["ssg_k_stats_bases"]["ms"] * 1e-3))
        if k.get("ssg_k_bgzf_inflate", {}).get("ms", 0) > 0:
            res["per_base_kernel_over_inflate"] = round(k["ssg_k_stats_bases"]["ms"] / k["ssg_k_bgzf_inflate"]["ms"], 3)
    if "kernel_resources" in kept:
        res["kernel_resources"] = kept["kernel_resources"]
    res["not_measured"] = "other tiles and slabs than the default; files of other read lengths; the 8 M-pair leg"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("what", "kernel_resources")}), flush=True)
    td_obj.cleanup()
    return 0 if res["stats_equals_samtools_stats"] else 1


if __name__ == "__main__":
    sys.exit(main())
