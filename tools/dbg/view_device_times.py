#!/usr/bin/env python3
"""`sambamba view` with a filter, a count or a region, host path against device path (SSG_VIEW_DEVICE=1), on one box: the sorted main BAM of one library -- a run of
4 M simulated pairs through the reference's unmodified script on the product executables -- and four queries on it: `-c' of the whole file, `-c -F' with the usual
filter, and `-f bam -o' of a 1 Mb region and of a whole contig (both through the file's .bai).  Host and device alternate, three runs each after a warm-up; then one device run of every query
with SSG_PROF=1 for the kernels' times.  Wall times only, the box's own spread next to them; no ratio is asserted.  The result goes to
profiles/r12_view_device.json (--out names another place).
usage: view_device_times.py [--pairs N] [--ref-mbp M] [--threads T] [--reps R] [--out FILE]"""
import argparse
import gzip
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from speedseq_amd import capi  # noqa: E402

OURS = ("SSG_VIEW_DEVICE", "SSG_PROF", "SSG_DEBUG")
USUAL = "proper_pair and not duplicate and mapping_quality >= 20"


def run(cmd, extra, limit_s=600):
    env = {k: v for k, v in os.environ.items() if k not in OURS}
    env.update(extra)
    t = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=limit_s)
    t = time.perf_counter() - t
    if r.returncode != 0:
        raise SystemExit("%s failed (rc %d): %s" % (" ".join(cmd), r.returncode, r.stderr[-1500:]))
    return round(t, 3), r.stdout, [l for l in r.stderr.split("\n") if l.startswith("[sambamba]")]


def spread(v):
    return round((max(v) - min(v)) / min(v), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4000000)
    ap.add_argument("--ref-mbp", type=float, default=3100.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_view_device.json"))
    a = ap.parse_args()
    torch.cuda.init(); dev = torch.device("cuda", 0)
    lib = capi.Lib()
    ref, lens, _ = bench.synth_reference(int(a.ref_mbp * 1e6), 20150810, dev)
    names = bench.GRCH37_NAMES[:len(lens)]
    ctg_off = np.concatenate([[0], np.cumsum(lens)])[:-1]
    idx = lib.index_build_dev(ref.data_ptr(), int(ref.numel()), ctg_off, lens, names)
    td_obj = tempfile.TemporaryDirectory(dir="/dev/shm" if os.access("/dev/shm", os.W_OK) else None); td = td_obj.name
    prefix = os.path.join(td, "ref.fa")
    lib.index_save(idx, prefix); lib.index_destroy(idx)
    b = lambda n: os.path.join(ROOT, "bin", n)
    fq = os.path.join(td, "lib.fq")
    r = bench.simulate_pairs(ref, lens, a.pairs, 150, 1000, dev).cpu().numpy()
    bench.write_fastq(fq, r, 150, first_pair=0)
    leg = bench.script_leg(td, "lib", prefix, fq, a.pairs, a.threads, b("bwa"), b("samblaster"), b("sambamba"), sort_mem_gb=64, config_extra="export SSG_FUSED=1\n", limit_s=400)
    if leg.get("error") or leg.get("skipped"):
        raise SystemExit("the script leg failed: %s" % leg)
    os.remove(fq)
    del ref
    torch.cuda.empty_cache()
    bam, smb, t = leg["out"] + ".bam", b("sambamba"), str(a.threads)
    ctg = names[0]
    mid = int(lens[0]) // 2
    out = os.path.join(td, "out.bam")
    if not os.path.exists(bam + ".bai") or os.path.getmtime(bam + ".bai") < os.path.getmtime(bam):
        run([smb, "index", "-t", t, bam], {})
    queries = {"count": ["-c", bam], "count_filter": ["-c", "-F", USUAL, bam], "region_1mb": ["-f", "bam", "-o", out, bam, "%s:%d-%d" % (ctg, mid, mid + 999999)], "contig": ["-f", "bam", "-o", out, bam, ctg]}
    res = {"what": "sambamba view on the sorted main BAM of one library (%d simulated pairs, 2x150, %.0f Mbp reference, through the script): host path and device path "
                   "(SSG_VIEW_DEVICE=1) alternating after a warm-up, wall seconds.  The region queries read the chunks the file's .bai gives for them and write BAM "
                   "(-f bam -o); their outputs are compared by their inflated bytes" % (a.pairs, a.ref_mbp),
           "threads": a.threads, "host_cpu_quota": bench.host_cpu_quota(), "bam_bytes": os.path.getsize(bam), "queries": {k: " ".join(v[:-1] if v[-1] == bam else v).replace(td, ".") for k, v in queries.items()}}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    for q, args in queries.items():
        res[q] = {"host_s": [], "device_s": []}
        answers = {}
        for rep in range(a.reps + 1):                                   # (the first round warms the page cache and is not kept)
            for m, extra in (("host", {}), ("device", {"SSG_VIEW_DEVICE": "1", "SSG_DEBUG": "1"})):
                w, stdout, log = run([smb, "view", "-t", t] + args, extra)
                answers[m] = stdout if "-c" in args else gzip.decompress(open(out, "rb").read())
                if rep:
                    res[q]["%s_s" % m].append(w)
                if m == "device":
                    res[q]["device_log"] = [l for l in log if "view:" in l]
                bench.log("%s %s: %.2f s" % (q, m, w))
        res[q]["device_equals_host"] = answers["host"] == answers["device"]
        res[q]["host_spread"], res[q]["device_spread"] = spread(res[q]["host_s"]), spread(res[q]["device_s"])
        # the kernels, one run under SSG_PROF (HIP events around every launch: not a timed run)
        w, _, log = run([smb, "view", "-t", t] + args, {"SSG_VIEW_DEVICE": "1", "SSG_DEBUG": "1", "SSG_PROF": "1"})
        res[q]["device_prof"] = {"wall_s": w, "kernels": [l.split("kernel", 1)[1].strip() for l in log if ": kernel " in l]}
        save()
    bench.log(json.dumps({q: {k: v for k, v in res[q].items() if not k.endswith("_log") and not k.endswith("_prof")} for q in queries}))
    td_obj.cleanup()


if __name__ == "__main__":
    main()
