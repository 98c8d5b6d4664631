#!/usr/bin/env python3
"""`sambamba merge` and `sambamba index`, host path against device path (SSG_MERGE_DEVICE=1 / SSG_INDEX_DEVICE=1), on one box: the main BAMs of two
libraries -- two runs of 4 M simulated pairs each, together the size of the 8 M-pair run (not one BAM split in two), each through the reference's unmodified script on the product executables -- merged, and the merged file
indexed, host and device alternating three times each; then one run of each device path with SSG_PROF=1 for the kernels' times.  Wall times only, the
box's own spread next to them; no ratio is asserted.  The result goes to profiles/r10_merge_device.json (--out names another place).
usage: merge_device_times.py [--pairs N] [--ref-mbp M] [--threads T] [--reps R] [--out FILE]"""
import argparse
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

OURS = ("SSG_MERGE_DEVICE", "SSG_MERGE_WINDOW", "SSG_MERGE_POOL", "SSG_INDEX_DEVICE", "SSG_PROF", "SSG_DEBUG")


def run(cmd, extra, limit_s=600):
    env = {k: v for k, v in os.environ.items() if k not in OURS}
    env.update(extra)
    t = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=limit_s)
    t = time.perf_counter() - t
    if r.returncode != 0:
        raise SystemExit("%s failed (rc %d): %s" % (" ".join(cmd), r.returncode, r.stderr[-1500:]))
    return round(t, 3), [l for l in r.stderr.split("\n") if l.startswith("[sambamba]")]


def spread(v):
    return round((max(v) - min(v)) / min(v), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8000000)
    ap.add_argument("--ref-mbp", type=float, default=3100.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_merge_device.json"))
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
    half = a.pairs // 2
    halves, legs = [], []
    for k in range(2):                                                  # two libraries of pairs / 2 simulated pairs each
        fq = os.path.join(td, "lib%d.fq" % k)
        r = bench.simulate_pairs(ref, lens, half, 150, 1000 + k, dev).cpu().numpy()
        bench.write_fastq(fq, r, 150, first_pair=k * half)
        leg = bench.script_leg(td, "lib%d" % k, prefix, fq, half, a.threads, b("bwa"), b("samblaster"), b("sambamba"), sort_mem_gb=64,
                               config_extra="export SSG_FUSED=1\n", limit_s=400)
        if leg.get("error") or leg.get("skipped"):
            raise SystemExit("the script leg of library %d failed: %s" % (k, leg))
        os.remove(fq)
        for x in (".splitters.bam", ".discordants.bam"):
            for y in ("", ".bai"):
                if os.path.exists(leg["out"] + x + y):
                    os.remove(leg["out"] + x + y)
        halves.append(leg["out"] + ".bam")
        legs.append({"pairs": half, "wall_s": leg["wall_s"], "bam_bytes": leg["bam_bytes"][".bam"]})
        bench.log("library %d: %d pairs, main BAM %.2f GB in %.1f s" % (k, half, leg["bam_bytes"][".bam"] / 1e9, leg["wall_s"]))
    del ref
    torch.cuda.empty_cache()
    smb, t = b("sambamba"), str(a.threads)
    res = {"what": "sambamba merge of the main BAMs of two libraries (two runs of the script, %d simulated pairs together, 2x150, %.0f Mbp reference) and sambamba index of the merged file; "
                   "host path and device path alternating, wall seconds" % (a.pairs, a.ref_mbp),
           "threads": a.threads, "host_cpu_quota": bench.host_cpu_quota(), "libraries": legs,
           "merge_host_s": [], "merge_device_s": [], "index_host_s": [], "index_device_s": []}
    out = {m: os.path.join(td, "merged_%s.bam" % m) for m in ("host", "device")}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)

    def clear(p):
        for y in ("", ".bai", ".bai.ssg"):
            if os.path.exists(p + y):
                os.remove(p + y)
    for rep in range(a.reps):
        for m, extra in (("host", {}), ("device", {"SSG_MERGE_DEVICE": "1", "SSG_DEBUG": "1"})):
            clear(out[m])
            w, log = run([smb, "merge", "-t", t, out[m]] + halves, extra)
            res["merge_%s_s" % m].append(w)
            if m == "device":
                res["merge_device_log"] = [l for l in log if "merge:" in l]
            bench.log("merge %s: %.2f s" % (m, w))
    save()
    res["merged_bytes"] = {m: os.path.getsize(out[m]) for m in out}
    # the index the device merge wrote against the one the host `sambamba index' makes of the same file
    bai_dev_merge = open(out["device"] + ".bai", "rb").read()
    os.remove(out["device"] + ".bai"); os.remove(out["device"] + ".bai.ssg")
    run([smb, "index", "-t", t, out["device"]], {})
    res["bai_of_device_merge_equals_host_index"] = open(out["device"] + ".bai", "rb").read() == bai_dev_merge
    bais = {}
    for rep in range(a.reps):
        for m, extra in (("host", {}), ("device", {"SSG_INDEX_DEVICE": "1", "SSG_DEBUG": "1"})):
            if os.path.exists(out["host"] + ".bai"):
                os.remove(out["host"] + ".bai")
            w, log = run([smb, "index", "-t", t, out["host"]], extra)
            res["index_%s_s" % m].append(w)
            bais[m] = open(out["host"] + ".bai", "rb").read()
            if m == "device":
                res["index_device_log"] = [l for l in log if "index:" in l]
            bench.log("index %s: %.2f s" % (m, w))
    res["bai_device_equals_host"] = bais["host"] == bais["device"]
    save()
    for k in ("merge_host_s", "merge_device_s", "index_host_s", "index_device_s"):
        res[k.replace("_s", "_spread")] = spread(res[k])
    # the kernels, one run each under SSG_PROF (HIP events around every launch: not a timed run)
    clear(out["device"])
    w, log = run([smb, "merge", "-t", t, out["device"]] + halves, {"SSG_MERGE_DEVICE": "1", "SSG_DEBUG": "1", "SSG_PROF": "1"})
    res["merge_device_prof"] = {"wall_s": w, "kernels": [l.split("kernel", 1)[1].strip() for l in log if ": kernel " in l]}
    os.remove(out["host"] + ".bai")
    w, log = run([smb, "index", "-t", t, out["host"]], {"SSG_INDEX_DEVICE": "1", "SSG_DEBUG": "1", "SSG_PROF": "1"})
    res["index_device_prof"] = {"wall_s": w, "kernels": [l.split("kernel", 1)[1].strip() for l in log if ": kernel " in l]}
    save()
    bench.log(json.dumps({k: v for k, v in res.items() if not k.endswith("_log") and not k.endswith("_prof")}))
    td_obj.cleanup()


if __name__ == "__main__":
    main()
