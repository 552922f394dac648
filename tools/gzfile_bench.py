#!/usr/bin/env python3
"""flate_hip_gzfile_read on three gzip files made from the same S-text, against the call each kind of file had before.

    python tools/gzfile_bench.py [--mib 1024] [--level 6] [--reps 5] [--only ABC] [--workload text|random|mixed]
                                 [--stored-units]
    python tools/gzfile_bench.py --trace A --calls 3       (run under a kernel trace: gzfile_read alone, --calls times)
    python tools/gzfile_bench.py --steps KERNEL_STATS.csv --calls 3      (that trace's kernel times as per-step times)

Builds --mib MiB of S-text and compresses it with zlib at --level (on the CPU, once) into
  (A) ONE gzip member                       against flate_hip_inflate_one;
  (B) 16 members of --mib / 16 MiB each     nothing to compare with on the GPU: the piecewise decoder's rate is the
                                            README's;
  (C) --mib * 16 members of 64 KiB          against flate_hip_gzip_read.
Every file is put on the device and timed with device pointers, whole calls, best of --reps, the two calls of a pair
ALTERNATED on the same card (a, b, a, b, ...; the first call of each sizes the ctx's scratch and is not counted); the
output of every gzfile_read is compared with the input once.  Prints one JSON line; also written to $FLATE_OUT_ROOT
(default results/)/gzfile_bench.json.  --workload and --stored-units are tools/one_bench.py's: other plain bytes, and
the option "one_stored_units" (stored block headers start units too)."""
import argparse
import csv
import importlib
import json
import os
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
flate = importlib.import_module("moonbit-flate_amd")
from one_bench import workload  # noqa: E402

HEADER = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff"
# the kernels of a flate_hip_gzfile_read call by step (a prefix of the kernel's name; the rest are "other")
STEPS = [("FIND", ("one_count", "one_fill", "gzip_count", "gzip_fill", "chain_scan", "gzfile_init", "gzfile_bits")),
         ("PROBE", ("one_probe",)),
         ("LINK", ("gzfile_link", "chain_round", "gzfile_finish", "one_out_scan", "gzfile_members", "gzfile_rel")),
         ("TAIL", ("one_tail",)),
         ("COMPOSE", ("one_seek_compose", "one_seek_resolve", "gzfile_pieces")),
         ("DECODE", ("inflate_simt", "one_check")),
         ("VERIFY", ("checksum_", "gzfile_trailer", "gzfile_verdict", "copy_ctl"))]


def member(plain, level):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    p = plain.tobytes()
    return HEADER + co.compress(p) + co.flush() + struct.pack("<II", zlib.crc32(p), len(p) & 0xffffffff)


def make(plain, n_members, level):
    """plain as n_members gzip members of equal size (zlib releases the GIL: the members are compressed side by side)."""
    size = plain.size // n_members
    with ThreadPoolExecutor(max_workers=min(16, n_members)) as pool:
        chunk = max(1, n_members // 64)
        groups = [range(g, min(g + chunk, n_members)) for g in range(0, n_members, chunk)]
        parts = pool.map(lambda ks: b"".join(member(plain[k * size:(k + 1) * size], level) for k in ks), groups)
        return b"".join(parts)


def steps_of(path, calls):
    """A rocprofv3 kernel_stats CSV of `calls` flate_hip_gzfile_read calls -> {step: ms per call}."""
    out = {name: 0.0 for name, _ in STEPS}
    out["other"] = 0.0
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name, total = row["Name"], float(row["TotalDurationNs"])
            step = next((s for s, prefixes in STEPS if any(p in name for p in prefixes)), "other")
            out[step] += total / 1e6 / calls
    return {k: round(v, 3) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="ABC")
    ap.add_argument("--trace", default="")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--steps", default="")
    ap.add_argument("--workload", choices=("text", "random", "mixed"), default="text")
    ap.add_argument("--stored-units", action="store_true")
    a = ap.parse_args()
    if a.steps:
        print(json.dumps({"per_call_ms": steps_of(a.steps, a.calls), "calls": a.calls}))
        return
    import torch

    plain = workload(a.workload, a.mib)
    counts = {"A": 1, "B": 16, "C": a.mib * 16}
    eng = flate.FlateEngine(0)
    eng.set_option("one_stored_units", 1 if a.stored_units else 0)
    out = torch.empty(plain.size + 16, dtype=torch.uint8, device="cuda")
    want = torch.from_numpy(plain)
    res = {"what": "gzip files of one S-text, device pointers, whole calls, ms, pairs alternated", "plain_bytes": int(plain.size),
           "zlib_level": a.level, "reps": a.reps, "workload": a.workload, "one_stored_units": int(a.stored_units),
           "build_id": flate.build_id()}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()  # (every call ends with a read-back of its result words behind a synchronise)
        return r, (time.perf_counter() - t0) * 1e3

    for key in (a.trace or a.only):
        t0 = time.perf_counter()
        f = make(plain, counts[key], a.level)
        d = torch.from_numpy(np.frombuffer(f, np.uint8).copy()).cuda()
        print("%s: %d members, %d bytes, compressed in %.1f s" % (key, counts[key], len(f), time.perf_counter() - t0),
              file=sys.stderr, flush=True)
        ours = lambda: eng.gzfile_read(d, out=out)[1]
        if a.trace:
            for _ in range(a.calls):
                r, _ = timed(ours)
                assert r.rc == 0 and r.out_len == plain.size, r
            continue
        theirs = {"A": lambda: eng.inflate_one(d, "gzip", out=out)[1], "B": None,
                  "C": lambda: eng.gzip_read(d, out=out)[1]}[key]
        t_ours, t_theirs = [], []
        for rep in range(a.reps + 1):
            r, t = timed(ours)
            assert r.rc == 0 and r.out_len == plain.size and r.n_members == counts[key], r
            if rep == 0:
                assert bool((out[:plain.size].cpu() == want).all()), "the output is not the input"
            t_ours.append(round(t, 3))
            if theirs:
                q, t = timed(theirs)
                assert q.rc == 0 and q.out_len == plain.size, q
                t_theirs.append(round(t, 3))
        row = {"members": counts[key], "file_bytes": len(f), "n_units": r.n_units, "n_candidates": r.n_candidates,
               "gzfile_read_ms_best": min(t_ours[1:]), "gzfile_read_ms_all": t_ours,
               "gzfile_read_gib_per_s": round(plain.size / 2**30 / (min(t_ours[1:]) * 1e-3), 3)}
        if theirs:
            row.update({"against": {"A": "inflate_one", "C": "gzip_read"}[key], "against_ms_best": min(t_theirs[1:]),
                        "against_ms_all": t_theirs, "ratio": round(min(t_ours[1:]) / min(t_theirs[1:]), 3)})
        res[key] = row
        print(json.dumps({key: row}), file=sys.stderr, flush=True)
        del d
    eng.close()
    if a.trace:
        return
    line = json.dumps(res)
    print(line)
    out_root = os.environ.get("FLATE_OUT_ROOT", os.path.join(ROOT, "results"))
    os.makedirs(out_root, exist_ok=True)
    with open(os.path.join(out_root, "gzfile_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
