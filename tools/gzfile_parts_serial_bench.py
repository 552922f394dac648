#!/usr/bin/env python3
"""A gzip FILE read in PARTS with short members decoded WHOLE (GzFileReader.set_serial_max) against the same reader
with S = 0 and against the whole-file calls.

    python tools/gzfile_parts_serial_bench.py [--mib 1024] [--level 6] [--reps 5] [--part 64] [--serial-max 1048576]
                                              [--only C,A,B,M1,M2] [--s0-only] [--cache DIR]

The input is --mib MiB of S-text compressed with zlib at --level (on the CPU, once per workload, the members in
parallel), resident on the device, as
  C   members of 64 KiB                    the reader with S on and with S = 0; against flate_hip_gzip_read and
                                           flate_hip_gzfile_read with the option "gzfile_serial_max" = S, whole
  A   ONE member                           S on against S = 0: the price of phase 1 per part
  B   16 members of --mib / 16 MiB         the same
  M1  8 members of --mib / 16 MiB in front of members of 64 KiB (half of the text each); M2: the other order
A PASS reads the whole file through the reader in parts of --part MiB of compressed bytes (a part begins where the last
call's in_used ends: a slice of the resident file, nothing is moved) into one output buffer of 4 parts, with device
pointers.  Per workload: best of --reps passes with lowest - highest, the variants ALTERNATED in this process on the
same card; the first round, which sizes the scratch, is not counted.  --s0-only: the S = 0 reader alone on every
workload (for a comparison between two builds of the library, FLATE_HIP_LIB; --cache DIR keeps the compressed files
between such runs).  Host pointers and per-step times are not measured.  Prints one JSON line; also written to
$FLATE_OUT_ROOT (default results/)/gzfile_parts_serial_bench.json."""
import argparse
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
flate = importlib.import_module("moonbit-flate_amd")
MIB = 1 << 20


def member(plain, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    raw = c.compress(plain) + c.flush()
    return flate.engine.GZIP_HEADER + raw + struct.pack("<II", zlib.crc32(plain), len(plain) & 0xffffffff)


def make_file(plain, member_bytes, level):
    """The members of member_bytes plain bytes each, in file order."""
    cuts = list(range(0, len(plain), member_bytes))
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:  # (zlib releases the interpreter's lock)
        return list(ex.map(lambda a: member(plain[a:a + member_bytes], level), cuts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--part", type=int, default=64)
    ap.add_argument("--serial-max", type=int, default=1 << 20)
    ap.add_argument("--only", default="C,A,B,M1,M2")
    ap.add_argument("--s0-only", action="store_true")
    ap.add_argument("--cache")
    a = ap.parse_args()
    import torch

    plain = memoryview(flate.synth("text", a.mib * 16, 65536).tobytes())
    T = len(plain)
    eng = flate.FlateEngine(0)
    whole_out = torch.empty(T + 16, dtype=torch.uint8, device="cuda")
    part = a.part * MIB
    out = torch.empty(4 * part, dtype=torch.uint8, device="cuda")
    res = {"what": "gzip files of S-text, whole passes, ms, device pointers, parts of %d MiB" % a.part, "plain_bytes": T,
           "zlib_level": a.level, "reps": a.reps, "serial_max": a.serial_max, "build_id": flate.build_id(),
           "not_measured": ["host pointers", "per-step times"]}

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, round((time.perf_counter() - t) * 1e3, 3)

    def stats(t):  # (the first round sizes the scratch)
        t = t[1:] if len(t) > 1 else t
        return {"ms_best": min(t), "ms_lowest_highest": [min(t), max(t)], "ms_all": t}

    def gz_pass(d, n, S, check):
        """The whole file through the gzip file reader -> (calls, members, whole members, units)."""
        rd = eng.open_gzfile_reader(device=True, serial_max=S) if S else eng.open_gzfile_reader(device=True)
        pos, calls, total, members, serial, units = 0, 0, 0, 0, 0, 0
        while True:
            end = min(pos + part, n)
            used, got, r = rd.read(d[pos:end], final=end == n, out=out)
            calls += 1
            assert r.rc in (0, 1) and (used or r.out_len), (r, pos)
            if check and calls == 2:
                assert bool((got == whole_out[total:total + r.out_len]).all())
            if S:
                serial += rd.last_route()[0]
            total, pos, members, units = total + r.out_len, pos + used, members + r.n_members, units + r.n_units
            if r.rc == 1:
                break
        rd.close()
        assert total == T and pos == n, (total, pos)
        return calls, members, serial, units

    def whole(d, S):
        eng.set_option("gzfile_serial_max", S)
        try:
            _, q = eng.gzfile_read(d, out=whole_out)
        finally:
            eng.set_option("gzfile_serial_max", 0)
        assert q.rc == 0 and q.out_len == T, q
        return q

    half = T // 2
    long_bytes = max(T // 16, 65536)
    for name in a.only.split(","):
        t0 = time.perf_counter()
        kept = os.path.join(a.cache, "%s_%d_%d.gz" % (name, a.mib, a.level)) if a.cache else None
        if kept and os.path.exists(kept):
            f = open(kept, "rb").read()
        else:
            if name in ("A", "B", "C"):
                ms = make_file(plain, {"A": T, "B": long_bytes, "C": 65536}[name], a.level)
            elif name == "M1":
                ms = make_file(plain[:half], long_bytes, a.level) + make_file(plain[half:], 65536, a.level)
            else:
                ms = make_file(plain[:half], 65536, a.level) + make_file(plain[half:], long_bytes, a.level)
            f = b"".join(ms)
            if kept:
                os.makedirs(a.cache, exist_ok=True)
                open(kept, "wb").write(f)
        n = len(f)
        d = torch.from_numpy(np.frombuffer(f, np.uint8).copy()).cuda()
        del f
        print("%s: %d bytes, ready in %.1f s" % (name, n, time.perf_counter() - t0), file=sys.stderr, flush=True)
        w = res[name] = {"file_bytes": n}
        q = whole(d, 0)  # (the truth the second call of a pass is held against)
        w["members"], w["walk_units"] = q.n_members, q.n_units
        t_on, t_off, t_whole, t_gzip = [], [], [], []
        for rep in range(a.reps + 1):
            if not a.s0_only:
                (calls, members, serial, units), t = timed(lambda: gz_pass(d, n, a.serial_max, rep == 0))
                t_on.append(t)
                w["reader_S"] = {"calls": calls, "serial_members": serial, "n_units": units}
                assert members == q.n_members
            (calls, members, _, units), t = timed(lambda: gz_pass(d, n, 0, rep == 0))
            t_off.append(t)
            w["reader_0"] = {"calls": calls, "n_units": units}
            assert members == q.n_members and units == q.n_units
            if name == "C" and not a.s0_only:
                t_whole.append(timed(lambda: whole(d, a.serial_max))[1])
                t_gzip.append(timed(lambda: eng.gzip_read(d, out=whole_out))[1])
        if t_on:
            w["reader_S"].update(stats(t_on))
        w["reader_0"].update(stats(t_off))
        if t_whole:
            w["gzfile_read_option_S"], w["gzip_read"] = stats(t_whole), stats(t_gzip)
        print(json.dumps({name: w}), file=sys.stderr, flush=True)
        del d
    eng.close()
    line = json.dumps(res)
    print(line)
    out_root = os.environ.get("FLATE_OUT_ROOT", os.path.join(ROOT, "results"))
    os.makedirs(out_root, exist_ok=True)
    with open(os.path.join(out_root, "gzfile_parts_serial_bench.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
