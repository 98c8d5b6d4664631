#!/usr/bin/env python3
"""`sambamba markdup' and `sambamba markdup -r' on one box: a coordinate-sorted BAM of N simulated pairs (2x150, the recipe of stats_times.py; every 50th pair
lies on the ends of the pair before it with lower qualities, so it is a duplicate by the rule) made with the project's own `sambamba view' and `sort'; wall
seconds of the whole command, two kept runs each after a warm-up run.  One more run under SSG_PROF=1 gives the kernels' times.  The summary line's counts are
held against what the recipe put in.  No duplicate marker of the reference tree follows this rule (`samtools rmdup' has another), so nothing is compared and no
ratio is asserted: a tool, not a test.  Everything goes to profiles/markdup_times.json (--out names another place).
usage: markdup_times.py [--pairs N] [--threads T] [--out FILE] [--sambamba PATH]"""
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
OURS = ("SSG_MARKDUP_BATCH", "SSG_PROF", "SSG_DEBUG", "SSG_BAM_LEVEL")
CTG = [("chr%d" % (i + 1), 40000000) for i in range(8)]
DEFAULT_OUT = os.path.join(ROOT, "profiles", "markdup_times.json")


def write_sam(path, n, seed=7):
    rng = np.random.RandomState(seed)
    with open(path, "wb") as f:
        f.write(("@HD\tVN:1.3\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CTG) + "@RG\tID:g1\tSM:s\tLB:l1\n").encode())
        seqs = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.choice(5, size=(2 * n, 150), p=[0.245, 0.25, 0.25, 0.245, 0.01])]
        quals = (33 + rng.choice([40, 40, 37, 25, 12, 2], size=(2 * n, 150))).astype(np.uint8)
        ctg = rng.randint(len(CTG), size=n); pos = rng.randint(1, CTG[0][1] - 1000, size=n); ins = rng.randint(200, 600, size=n)
        out = []
        for i in range(n):
            dup = i % 50 == 0 and i > 0
            j = i - 1 if dup else i                                       # a duplicate lies on the ends of the pair before it
            name, c = b"sim_%d" % i, CTG[ctg[j]][0].encode()
            p1, p2 = int(pos[j]), int(pos[j] + ins[j])
            q1, q2 = (b"#" * 150, b"#" * 150) if dup else (quals[2 * i].tobytes(), quals[2 * i + 1].tobytes())
            out.append(b"%s\t99\t%s\t%d\t60\t150M\t=\t%d\t%d\t%s\t%s\tRG:Z:g1\n" % (name, c, p1, p2, p2 - p1 + 150, seqs[2 * i].tobytes(), q1))
            out.append(b"%s\t147\t%s\t%d\t60\t150M\t=\t%d\t%d\t%s\t%s\tRG:Z:g1\n" % (name, c, p2, p1, p1 - p2 - 150, seqs[2 * i + 1].tobytes(), q2))
        f.write(b"".join(out))
    return (n - 1) // 50


def run(cmd, extra, limit_s=1500):
    env = {k: v for k, v in os.environ.items() if k not in OURS}
    env.update(extra)
    t = time.perf_counter()
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=limit_s)
    t = time.perf_counter() - t
    if r.returncode != 0:
        raise SystemExit("%s failed (rc %d): %s" % (" ".join(cmd), r.returncode, r.stderr[-1500:]))
    return round(t, 3), r.stderr.split("\n")


def kernels(log):
    out = {}
    for l in log:
        m = re.search(r": kernel (\S+)\s+([0-9.]+) ms in (\d+) launches", l)
        if m:
            out[m.group(1)] = {"ms": float(m.group(2)), "launches": int(m.group(3))}
    return out


def summary(log):
    for l in log:
        m = re.search(r"markdup: (\d+) records, (\d+) taking part, (\d+) pairs, (\d+) unmatched paired, (\d+) fragments, (\d+) duplicates found", l)
        if m:
            return dict(zip(("records", "taking_part", "pairs", "unmatched", "fragments", "duplicates"), (int(x) for x in m.groups())))
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=200000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--sambamba", default=os.path.join(ROOT, "bin", "sambamba"), help="another build of the executable (tests/emu/sambamba_emu: the host emulation, to try the tool without a device)")
    a = ap.parse_args()
    sambamba = a.sambamba
    td_obj = tempfile.TemporaryDirectory(); td = td_obj.name
    sam, ubam, bam = td + "/in.sam", td + "/in.u.bam", td + "/in.bam"
    t = time.perf_counter()
    n_dup_pairs = write_sam(sam, a.pairs)
    clean = {k: v for k, v in os.environ.items() if k not in OURS}
    with open(sam, "rb") as fi, open(ubam, "wb") as fo:
        subprocess.run([sambamba, "view", "-S", "-f", "bam", "/dev/stdin"], stdin=fi, stdout=fo, check=True, env=clean)
    os.remove(sam)
    subprocess.run([sambamba, "sort", "-t", str(a.threads), "-m", "32G", "--tmpdir=%s/tmp" % td, "-o", bam, ubam], check=True, capture_output=True, env=clean)
    os.remove(ubam)
    print("input made in %.0f s: %d bytes" % (time.perf_counter() - t, os.path.getsize(bam)), flush=True)
    res = {"what": "sambamba markdup and markdup -r (device) on a coordinate-sorted BAM of %d simulated pairs (2x150, one read group, every 50th pair a duplicate of the pair before it) "
                   "over 8 contigs of 40 Mb; wall seconds of the whole command, output file included; the first run of each warms the page cache and is not kept" % a.pairs,
           "pairs": a.pairs, "threads_of_the_box": os.cpu_count(), "bam_bytes": os.path.getsize(bam), "duplicate_pairs_put_in": n_dup_pairs}
    jobs = {"markdup": [sambamba, "markdup", "-t", str(a.threads), bam, td + "/out.bam"], "markdup_r": [sambamba, "markdup", "-r", "-t", str(a.threads), bam, td + "/out_r.bam"]}
    for name in jobs:
        res[name + "_s"] = []
    for rep in range(3):
        for name, cmd in jobs.items():
            w, log = run(cmd, {})
            if rep:
                res[name + "_s"].append(w)
            res[name + "_summary"] = summary(log)
            print("%s: %.2f s" % (name, w), flush=True)
    res["records_per_s"] = round(2 * a.pairs / min(res["markdup_s"]))
    res["out_bytes"] = {"markdup": os.path.getsize(td + "/out.bam"), "markdup_r": os.path.getsize(td + "/out_r.bam")}
    s = res["markdup_summary"]
    res["counts_are_the_recipes"] = bool(s) and s["records"] == 2 * a.pairs and s["pairs"] == a.pairs and s["duplicates"] >= 2 * n_dup_pairs
    w, log = run(jobs["markdup"], {"SSG_PROF": "1"})                                                               # (HIP events around every launch: not a timed run)
    res["prof"] = {"wall_s": w, "kernels": kernels(log)}
    res["not_measured"] = "no other duplicate marker ran on this input: none in the reference tree follows this rule; unsorted input; several libraries; files of other read lengths; batches other than the default"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "what"}), flush=True)
    td_obj.cleanup()
    return 0 if res["counts_are_the_recipes"] else 1


if __name__ == "__main__":
    sys.exit(main())
