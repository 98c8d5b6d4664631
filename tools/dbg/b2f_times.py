#!/usr/bin/env python3
"""`bamkit bamtofastq', host path against device path (SSG_B2F_DEVICE=1), on one box: a coordinate-sorted BAM of N simulated pairs (2x150, two read groups, a
secondary record now and then) made with the project's own `sambamba view' and `sambamba sort', then both paths on it, the device path once more under SSG_PROF=1
for the kernels' times.  The outputs must be equal (sha256).  Both wall times, the device path's closing line, the text kernel's bytes per second and what a
device-to-device copy of as many bytes reaches on the same box go to profiles/b2f_times.json (--out names another place).  A tool, not a test: no ratio is
asserted.
usage: b2f_times.py [--pairs N] [--threads T] [--out FILE]"""
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
OURS = ("SSG_B2F_DEVICE", "SSG_B2F_POOL", "SSG_B2F_BATCH", "SSG_PROF", "SSG_DEBUG")
CTG = [("chr%d" % (i + 1), 40000000) for i in range(8)]


def write_sam(path, n, seed=7):
    rng = np.random.RandomState(seed)
    with open(path, "wb") as f:
        f.write(("@HD\tVN:1.3\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CTG) + "@RG\tID:lib1\tSM:s\n@RG\tID:lib2\tSM:s\n").encode())
        step = 50000
        for a in range(0, n, step):
            m = min(step, n - a)
            seqs = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, size=(2 * m, 150))]
            quals = (33 + rng.choice([40, 40, 37, 25, 12, 2], size=(2 * m, 150))).astype(np.uint8)
            ctg = rng.randint(len(CTG), size=m); pos = rng.randint(1, CTG[0][1] - 1000, size=m); ins = rng.randint(200, 600, size=m)
            far = rng.randint(100, size=m) == 0                             # one pair in a hundred has its mate on another contig: the halves wait long
            out = []
            for i in range(m):
                name, rg = b"sim_%d" % (a + i), (b"lib1", b"lib2")[(a + i) & 1]
                c1 = CTG[ctg[i]][0].encode(); c2 = CTG[(ctg[i] + 3) % len(CTG)][0].encode() if far[i] else c1
                p1, p2 = int(pos[i]), int(pos[i] + ins[i])
                s1, s2, q1, q2 = seqs[2 * i].tobytes(), seqs[2 * i + 1].tobytes(), quals[2 * i].tobytes(), quals[2 * i + 1].tobytes()
                out.append(b"%s\t99\t%s\t%d\t60\t150M\t%s\t%d\t0\t%s\t%s\tNM:i:0\tRG:Z:%s\n" % (name, c1, p1, b"=" if c2 == c1 else c2, p2, s1, q1, rg))
                out.append(b"%s\t147\t%s\t%d\t60\t150M\t%s\t%d\t0\t%s\t%s\tNM:i:1\tRG:Z:%s\n" % (name, c2, p2, b"=" if c2 == c1 else c1, p1, s2, q2, rg))
                if (a + i) % 97 == 0:
                    out.append(b"%s\t355\t%s\t%d\t0\t60H90M\t=\t%d\t0\t%s\t%s\tRG:Z:%s\n" % (name, c1, p1 + 11, p2, s1[60:], q1[60:], rg))
            f.write(b"".join(out))


def run(cmd, extra, stdout, limit_s=900):
    env = {k: v for k, v in os.environ.items() if k not in OURS}
    env.update(extra)
    t = time.perf_counter()
    with open(stdout, "wb") as fo:
        r = subprocess.run(cmd, stdout=fo, stderr=subprocess.PIPE, text=True, env=env, timeout=limit_s)
    t = time.perf_counter() - t
    if r.returncode != 0:
        raise SystemExit("%s failed (rc %d): %s" % (" ".join(cmd), r.returncode, r.stderr[-1500:]))
    return round(t, 3), r.stderr.split("\n")


def sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


def d2d_copy_rate(n_bytes):
    """bytes per second of a device-to-device copy of n_bytes (the best of five after a warm-up)"""
    import torch
    a = torch.empty(n_bytes, dtype=torch.uint8, device="cuda"); b = torch.empty_like(a)
    b.copy_(a); torch.cuda.synchronize()
    best = None
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); b.copy_(a); e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return n_bytes / (best * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2000000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "b2f_times.json"))
    a = ap.parse_args()
    b = lambda n: os.path.join(ROOT, "bin", n)
    td_obj = tempfile.TemporaryDirectory(); td = td_obj.name
    sam, ubam, bam = td + "/in.sam", td + "/in.u.bam", td + "/in.bam"
    t = time.perf_counter()
    write_sam(sam, a.pairs)
    clean = {k: v for k, v in os.environ.items() if k not in OURS}
    with open(sam, "rb") as fi, open(ubam, "wb") as fo:
        subprocess.run([b("sambamba"), "view", "-S", "-f", "bam", "/dev/stdin"], stdin=fi, stdout=fo, check=True, env=clean)
    os.remove(sam)
    subprocess.run([b("sambamba"), "sort", "-t", str(a.threads), "-m", "32G", "--tmpdir=%s/tmp" % td, "-o", bam, ubam], check=True, capture_output=True, env=clean)
    os.remove(ubam)
    print("input made in %.0f s: %d bytes" % (time.perf_counter() - t, os.path.getsize(bam)), flush=True)
    cmd = [b("bamkit"), "bamtofastq", bam]
    res = {"what": "bamkit bamtofastq on a coordinate-sorted BAM of %d simulated pairs (2x150, two read groups, one pair in a hundred across contigs, a hard-clipped secondary "
                   "record per 97 pairs): the host path and the device path (SSG_B2F_DEVICE=1), wall seconds of the whole command with the text written to a file; the "
                   "first run of each warms the page cache and is not kept" % a.pairs,
           "pairs": a.pairs, "threads_of_the_box": os.cpu_count(), "bam_bytes": os.path.getsize(bam), "host_s": [], "device_s": []}
    for rep in range(3):
        for m, extra in (("host", {}), ("device", {"SSG_B2F_DEVICE": "1", "SSG_DEBUG": "1"})):
            w, log = run(cmd, extra, "%s/%s.fq" % (td, m))
            if rep:
                res["%s_s" % m].append(w)
            if m == "device":
                res["device_log"] = [l for l in log if "bamtofastq" in l]
            print("%s: %.2f s" % (m, w), flush=True)
    res["fastq_bytes"] = os.path.getsize(td + "/host.fq")
    res["sha256_host"], res["sha256_device"] = sha256(td + "/host.fq"), sha256(td + "/device.fq")
    res["device_equals_host"] = res["sha256_host"] == res["sha256_device"]
    res["device_ran"] = any("on the device" in l for l in res["device_log"])
    w, log = run(cmd, {"SSG_B2F_DEVICE": "1", "SSG_DEBUG": "1", "SSG_PROF": "1"}, td + "/prof.fq")                                   # (HIP events around every launch: not a timed run)
    res["device_prof"] = {"wall_s": w, "kernels": [l.split("kernel", 1)[1].strip() for l in log if ": kernel " in l]}
    for l in res["device_prof"]["kernels"]:
        m = re.match(r"ssg_k_b2f_text\s+([0-9.]+) ms", l)
        if m and float(m.group(1)) > 0:
            res["text_kernel_ms"] = float(m.group(1))
            res["text_kernel_bytes_per_s"] = round(res["fastq_bytes"] / (float(m.group(1)) * 1e-3))
    try:
        res["d2d_copy_bytes_per_s"] = round(d2d_copy_rate(res["fastq_bytes"]))
    except Exception as e:                                                  # (the copy is a yardstick, not the measurement)
        res["d2d_copy_error"] = str(e)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("what", "device_prof")}), flush=True)
    td_obj.cleanup()
    return 0 if res["device_equals_host"] and res["device_ran"] else 1


if __name__ == "__main__":
    sys.exit(main())
