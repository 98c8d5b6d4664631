#!/usr/bin/env python3
"""Device time of ssg_bgzf_inflate's kernels next to the host reader's wall time on the same members (the numbers of
profiles/r08_bgzf_inflate.json).  4096 members of 0xff00 BAM-shaped bytes each, once deflated by zlib at level 6 and once by this library
(ssg_bgzf_compress); per input a warm-up and three repeats, the inputs alternating:
  - ssg_k_bgzf_inflate and ssg_k_crc32_ranges by ssg_prof_get around one ssg_bgzf_inflate call, and the call's wall time (copies included);
  - tools/dbg/inflate_probe on a file of the same members: bgzf_in_t::next_batch with zlib on 16 threads (the path every reader takes
    today), and with the batch-inflate hook.
usage: inflate_times.py [--members 4096] [--threads 16] [--out FILE] [--probe tools/dbg/inflate_probe]"""
import ctypes as C
import json
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from speedseq_amd import capi  # noqa: E402


def bam_stream(n_bytes, seed=11):
    """BAM-shaped records: core, name, CIGAR, packed bases, qualities of few values, tags"""
    rng = np.random.RandomState(seed)
    recs, total = [], 0
    tags = b"NMC\x00MDZ150\x00ASC\x96XSC\x00RGZgrp1\x00MCZ150M\x00MQC\x3c"
    while total < n_bytes:
        name = b"read%d\0" % rng.randint(10 ** 7)
        core = struct.pack("<iiIIiiii", rng.randint(25), rng.randint(10 ** 8), 0x12345678, (99 << 16) | 1, 150, rng.randint(25), rng.randint(10 ** 8), rng.randint(-500, 500))
        body = core + name + struct.pack("<I", 150 << 4) + rng.bytes(75) + rng.choice(np.array([40, 40, 40, 37, 12], dtype=np.uint8), 150).tobytes() + tags
        recs.append(struct.pack("<I", len(body)) + body)
        total += len(recs[-1])
    return b"".join(recs)[:n_bytes]


def member(stream, payload):
    total = 18 + len(stream) + 8
    return bytes.fromhex("1f8b08040000000000ff060042430200") + struct.pack("<H", total - 1) + stream + struct.pack("<II", zlib.crc32(payload), len(payload))


def main():
    arg = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d
    n, threads, out_path = int(arg("--members", "4096")), int(arg("--threads", "16")), arg("--out", "")
    probe = arg("--probe", os.path.join(ROOT, "tools", "dbg", "inflate_probe"))
    lib = capi.Lib()
    pool = bam_stream(32 << 20)                                           # the members are windows of 32 MB of records, each starting elsewhere
    step = (len(pool) - 0xff00) // n
    payloads = [pool[k * step:k * step + 0xff00] for k in range(n)]

    def z6(p):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        return member(c.compress(p) + c.flush(), p)
    with ThreadPoolExecutor(16) as ex:
        zmem = list(ex.map(z6, payloads))
    blob = np.frombuffer(b"".join(payloads), dtype=np.uint8)
    cut = np.arange(n + 1, dtype=np.uint64) * 0xff00
    own, own_off, _ = capi.bgzf_compress(lib, blob, cut)
    inputs = {"zlib level 6": (np.frombuffer(b"".join(zmem), dtype=np.uint8), np.concatenate([[0], np.cumsum([len(m) for m in zmem])]).astype(np.uint64)),
              "this library's deflate": (own, own_off)}
    res = {"members": n, "payload_bytes": int(blob.size), "threads": threads, "inputs": {}}
    files = {}
    tmp = tempfile.mkdtemp(prefix="inflate_times_")
    for name, (mem, off) in inputs.items():
        files[name] = os.path.join(tmp, "%d.bgzf" % len(files))
        open(files[name], "wb").write(mem.tobytes())
        res["inputs"][name] = {"member_bytes": int(off[-1]), "device_calls": [], "reader_zlib": [], "reader_device": []}
    lib.l.ssg_prof_enable(C.c_int(1))
    for rep in range(4):                                                  # the first is the warm-up
        for name, (mem, off) in inputs.items():
            lib.l.ssg_prof_reset()
            t0 = time.perf_counter()
            rc, out, ooff, st = capi.bgzf_inflate(lib, mem, off)
            wall = time.perf_counter() - t0
            assert rc == 0 and (st == 0).all() and out.tobytes() == blob.tobytes()
            prof = capi.prof_get(lib)
            row = {"wall_s": round(wall, 4), "kernels_ms": dict((k, round(v[0], 3)) for k, v in prof.items()), "warm_up": rep == 0}
            res["inputs"][name]["device_calls"].append(row)
    for name in inputs:                                                   # the readers: one process per input, zlib and the hook alternating, the first pair the warm-up
        r = subprocess.run([probe, files[name], str(threads), "2", "4"], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr
        for line in r.stdout.strip().split("\n"):
            j = json.loads(line)
            assert j["payload_bytes"] == blob.size and j["hook_kept"]
            j["warm_up"] = j["repeat"] == 0
            res["inputs"][name]["reader_device" if j["device"] else "reader_zlib"].append(j)
    lib.l.ssg_prof_enable(C.c_int(0))
    for f in files.values(): os.unlink(f)
    os.rmdir(tmp)
    text = json.dumps(res, indent=1)
    print(text)
    if out_path:
        open(out_path, "w").write(text + "\n")


if __name__ == "__main__":
    main()
