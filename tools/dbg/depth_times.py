#!/usr/bin/env python3
"""`sambamba depth' against the reference's samtools 1.3.1 (oracle/_ref/samtools) on one box: a coordinate-sorted, indexed BAM of N simulated pairs (2x150) made
with the project's own `sambamba view', `sort' and `index'; `depth base' against `samtools depth' and `depth window -w 1000' against `samtools bedcov' on a BED of
the same 1000-base windows, two alternating runs each after a warm-up, the outputs compared (sha256; of bedcov the four columns it has).  One more device run under
SSG_PROF=1 gives the kernels' times, and two give the accumulating kernel's records per second with the LDS tile on (the default) and off (SSG_DEPTH_TILE=0).
Everything goes to profiles/depth_times.json (--out names another place).  A tool, not a test: no ratio is asserted.
usage: depth_times.py [--pairs N] [--threads T] [--out FILE]"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OURS = ("SSG_DEPTH_SPAN", "SSG_DEPTH_TILE", "SSG_PROF", "SSG_DEBUG")
CTG = [("chr%d" % (i + 1), 40000000) for i in range(8)]
SAMTOOLS = os.path.join(ROOT, "oracle", "_ref", "samtools")


def write_sam(path, n, seed=7):
    rng = np.random.RandomState(seed)
    with open(path, "wb") as f:
        f.write(("@HD\tVN:1.3\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CTG)).encode())
        step = 50000
        for a in range(0, n, step):
            m = min(step, n - a)
            seqs = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, size=(2 * m, 150))]
            quals = (33 + rng.choice([40, 40, 37, 25, 12, 2], size=(2 * m, 150))).astype(np.uint8)
            ctg = rng.randint(len(CTG), size=m); pos = rng.randint(1, CTG[0][1] - 1000, size=m); ins = rng.randint(200, 600, size=m)
            out = []
            for i in range(m):
                name, c = b"sim_%d" % (a + i), CTG[ctg[i]][0].encode()
                p1, p2 = int(pos[i]), int(pos[i] + ins[i])
                cig = b"150M" if (a + i) % 9 else b"70M2D80M"
                out.append(b"%s\t99\t%s\t%d\t60\t%s\t=\t%d\t0\t%s\t%s\n" % (name, c, p1, cig, p2, seqs[2 * i].tobytes(), quals[2 * i].tobytes()))
                out.append(b"%s\t%d\t%s\t%d\t60\t150M\t=\t%d\t0\t%s\t%s\n" % (name, 147 | (1024 if (a + i) % 50 == 0 else 0), c, p2, p1, seqs[2 * i + 1].tobytes(), quals[2 * i + 1].tobytes()))
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


def sha256(path, columns=None):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        if columns is None:
            for blk in iter(lambda: f.read(1 << 24), b""):
                h.update(blk)
        else:
            for l in f:
                h.update(b"\t".join(l.rstrip(b"\n").split(b"\t")[:columns]) + b"\n")
    return h.hexdigest()


def kernels(log):
    out = {}
    for l in log:
        m = re.search(r": kernel (\S+)\s+([0-9.]+) ms in (\d+) launches", l)
        if m:
            out[m.group(1)] = {"ms": float(m.group(2)), "launches": int(m.group(3))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2000000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_times.json"))
    a = ap.parse_args()
    sambamba = os.path.join(ROOT, "bin", "sambamba")
    if not os.path.exists(SAMTOOLS):
        raise SystemExit("%s is not there: __graft_entry__.build() makes it from the reference" % SAMTOOLS)
    td_obj = tempfile.TemporaryDirectory(); td = td_obj.name
    sam, ubam, bam, bed = td + "/in.sam", td + "/in.u.bam", td + "/in.bam", td + "/windows.bed"
    t = time.perf_counter()
    write_sam(sam, a.pairs)
    clean = {k: v for k, v in os.environ.items() if k not in OURS}
    with open(sam, "rb") as fi, open(ubam, "wb") as fo:
        subprocess.run([sambamba, "view", "-S", "-f", "bam", "/dev/stdin"], stdin=fi, stdout=fo, check=True, env=clean)
    os.remove(sam)
    subprocess.run([sambamba, "sort", "-t", str(a.threads), "-m", "32G", "--tmpdir=%s/tmp" % td, "-o", bam, ubam], check=True, capture_output=True, env=clean)
    os.remove(ubam)
    subprocess.run([sambamba, "index", "-t", str(a.threads), bam], check=True, capture_output=True, env=clean)
    with open(bed, "w") as f:
        for name, ln in CTG:
            f.write("".join("%s\t%d\t%d\n" % (name, w, min(w + 1000, ln)) for w in range(0, ln, 1000)))
    print("input made in %.0f s: %d bytes" % (time.perf_counter() - t, os.path.getsize(bam)), flush=True)
    res = {"what": "sambamba depth (device) against samtools 1.3.1 (host, one thread) on a coordinate-sorted BAM of %d simulated pairs (2x150, a 2D in one read of nine, "
                   "a duplicate per 50 pairs) over 8 contigs of 40 Mb: `depth base' against `samtools depth', `depth window -w 1000' against `samtools bedcov' on the "
                   "same windows; wall seconds of the whole command with the output written to a file; the first run of each warms the page cache and is not kept" % a.pairs,
           "pairs": a.pairs, "threads_of_the_box": os.cpu_count(), "bam_bytes": os.path.getsize(bam)}
    jobs = {"base": [sambamba, "depth", "base", bam], "samtools_depth": [SAMTOOLS, "depth", bam],
            "window": [sambamba, "depth", "window", "-w", "1000", bam], "samtools_bedcov": [SAMTOOLS, "bedcov", bed, bam]}
    for name in jobs:
        res[name + "_s"] = []
    for rep in range(3):
        for name, cmd in jobs.items():
            w, _ = run(cmd, {}, "%s/%s.out" % (td, name))
            if rep:
                res[name + "_s"].append(w)
            print("%s: %.2f s" % (name, w), flush=True)
    res["base_bytes"] = os.path.getsize(td + "/base.out")
    res["base_equals_samtools_depth"] = sha256(td + "/base.out") == sha256(td + "/samtools_depth.out")
    res["window_equals_samtools_bedcov"] = sha256(td + "/window.out", 4) == sha256(td + "/samtools_bedcov.out", 4)
    w, log = run(jobs["base"], {"SSG_PROF": "1"}, td + "/prof.out")                                               # (HIP events around every launch: not a timed run)
    res["base_prof"] = {"wall_s": w, "kernels": kernels(log)}
    w, log = run(jobs["window"], {"SSG_PROF": "1"}, td + "/prof.out")
    res["window_prof"] = {"wall_s": w, "kernels": kernels(log)}
    n_used = 2 * a.pairs - (a.pairs + 49) // 50                                                                   # what the default filter keeps
    for tag, extra in (("tile_on", {}), ("tile_off", {"SSG_DEPTH_TILE": "0"}), ("tile_on_q20", {}), ("tile_off_q20", {"SSG_DEPTH_TILE": "0"})):
        w, log = run(jobs["base"][:3] + (["-q", "20"] if tag.endswith("q20") else []) + [bam], dict(extra, SSG_PROF="1"), td + "/prof.out")
        k = kernels(log).get("ssg_k_depth_accum")
        if k and k["ms"] > 0:
            res["accum_" + tag] = {"ms": k["ms"], "launches": k["launches"], "records_per_s": round(n_used / (k["ms"] * 1e-3))}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("what", "base_prof", "window_prof")}), flush=True)
    td_obj.cleanup()
    return 0 if res["base_equals_samtools_depth"] and res["window_equals_samtools_bedcov"] else 1


if __name__ == "__main__":
    sys.exit(main())
