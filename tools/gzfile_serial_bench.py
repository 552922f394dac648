#!/usr/bin/env python3
"""flate_hip_gzfile_read with the option "gzfile_serial_max" (short members decoded whole) against the same call with
the option off and, on a file of short members, against flate_hip_gzip_read.

    python tools/gzfile_serial_bench.py [--mib 1024] [--level 6] [--reps 5] [--serial-max 1048576]
                                        [--only ABCMXY] [--sweep 65536,262144,1048576,4194304]

Builds --mib MiB of S-text and compresses it with zlib at --level (on the CPU, once per member size) into
  (A) ONE gzip member;
  (B) 16 members of --mib / 16 MiB each;
  (C) --mib * 16 members of 64 KiB;
  (M) --mib members of 1 MiB;
  (X) the first half of the text as B's long members IN FRONT of the second half as C's short ones;
  (Y) the first half as C's short members in front of the second half as B's long ones.
Every file is put on the device and timed with device pointers, whole calls, best of --reps, the variants of a file
ALTERNATED on the same card (off, on, [gzip_read,] off, on, ...; the first call of each sizes the ctx's scratch and is
not counted); every variant's output is compared with the input once.  With the option on, the row carries
flate_hip_gzfile_last_route's words.  --sweep: on A and M, the option at each of these values as well.  Prints one JSON
line; also written to $FLATE_OUT_ROOT (default results/)/gzfile_serial_bench.json."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
flate = importlib.import_module("moonbit-flate_amd")
from gzfile_bench import member  # noqa: E402
from one_bench import workload  # noqa: E402


def members(plain, n_members, level):
    """plain as n_members gzip members of equal size -> the list of them (compressed side by side)."""
    from concurrent.futures import ThreadPoolExecutor
    size = plain.size // n_members
    with ThreadPoolExecutor(max_workers=min(16, n_members)) as pool:
        return list(pool.map(lambda k: member(plain[k * size:(k + 1) * size], level), range(n_members), chunksize=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--serial-max", type=int, default=1 << 20)
    ap.add_argument("--only", default="ABCMXY")
    ap.add_argument("--sweep", default="")
    a = ap.parse_args()
    import torch

    plain = workload("text", a.mib)
    sweep = [int(s) for s in a.sweep.split(",") if s]
    eng = flate.FlateEngine(0)
    out = torch.empty(plain.size + 16, dtype=torch.uint8, device="cuda")
    want = torch.from_numpy(plain)
    res = {"what": "gzip files of one S-text, device pointers, whole calls, ms, variants alternated",
           "plain_bytes": int(plain.size), "zlib_level": a.level, "reps": a.reps, "serial_max": a.serial_max,
           "build_id": flate.build_id()}
    made = {}

    def parts(n):
        if n not in made:
            t0 = time.perf_counter()
            made[n] = members(plain, n, a.level)
            print("%d members compressed in %.1f s" % (n, time.perf_counter() - t0), file=sys.stderr, flush=True)
        return made[n]

    def file_of(key):
        long_n, short_n = 16, a.mib * 16
        if key in "ABCM":
            return b"".join(parts({"A": 1, "B": long_n, "C": short_n, "M": a.mib}[key]))
        lo, sh = parts(long_n), parts(short_n)
        if key == "X":
            return b"".join(lo[:long_n // 2] + sh[short_n // 2:])
        return b"".join(sh[:short_n // 2] + lo[long_n // 2:])

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()  # (every call ends with a read-back of its result words behind a synchronise)
        return r, (time.perf_counter() - t0) * 1e3

    for key in a.only:
        f = file_of(key)
        d = torch.from_numpy(np.frombuffer(f, np.uint8).copy()).cuda()

        def gzfile(S):
            def call():
                eng.set_option("gzfile_serial_max", S)
                r = eng.gzfile_read(d, out=out)[1]
                eng.set_option("gzfile_serial_max", 0)
                return r
            return call

        variants = [("off", gzfile(0)), ("on", gzfile(a.serial_max))]
        if key in "AM":
            variants += [("on_%d" % s, gzfile(s)) for s in sweep if s != a.serial_max]
        if key == "C":
            variants.append(("gzip_read", lambda: eng.gzip_read(d, out=out)[1]))
        times = {name: [] for name, _ in variants}
        row = {"file_bytes": len(f)}
        for rep in range(a.reps + 1):
            for name, fn in variants:
                r, t = timed(fn)
                assert r.rc == 0 and r.out_len == plain.size, (key, name, r)
                times[name].append(round(t, 3))
                if rep == 0:
                    assert bool((out[:plain.size].cpu() == want).all()), "the output is not the input"
                    out.zero_()
                    if name != "gzip_read":
                        row[name + "_words"] = {"n_members": r.n_members, "n_units": r.n_units,
                                                "n_candidates": r.n_candidates}
                        eng.set_option("gzfile_serial_max", 0)
                        if name != "off":
                            S = a.serial_max if name == "on" else int(name[3:])
                            eng.set_option("gzfile_serial_max", S)
                            eng.gzfile_index(d, query=True)
                            sm, um, ff = eng.gzfile_last_route()
                            eng.set_option("gzfile_serial_max", 0)
                            row[name + "_words"].update({"serial_members": sm, "unit_members": um, "find_from": ff})
        for name, _ in variants:
            row[name + "_ms_best"] = min(times[name][1:])
            row[name + "_ms_all"] = times[name]
        res[key] = row
        print(json.dumps({key: row}), file=sys.stderr, flush=True)
        del d
    eng.close()
    line = json.dumps(res)
    print(line)
    out_root = os.environ.get("FLATE_OUT_ROOT", os.path.join(ROOT, "results"))
    os.makedirs(out_root, exist_ok=True)
    with open(os.path.join(out_root, "gzfile_serial_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
