#!/usr/bin/env python3
"""flate_hip_zip_read with the option "zip_unit_min" (long entries decoded through units) against the calls that do the
same work, on ZIP archives made from one S-text.

    python tools/zip_units_bench.py [--mib 1024] [--level 6] [--reps 5] [--only ABCDE] [--parent-lib PATH]

Builds --mib MiB of S-text and compresses it with zlib at --level (on the CPU, once per entry size) into archives with
local headers, a central directory and an end record (method 8, no Zip64: below 4 GiB and 65535 entries):
  (A) ONE entry of --mib MiB              option on against flate_hip_inflate_one (RAW) on the same stream: the same
                                          work, the difference is the price of the ZIP glue.  Option off is one
                                          wavefront on the whole entry: measured on ONE entry of 64 MiB instead.
  (B) 16 entries of --mib / 16 MiB        option on against flate_hip_gzfile_read on the same streams as gzip members;
  (C) --mib * 16 entries of 64 KiB        threshold 1 against option 0: the cost on small entries;
  (D) --mib MiB as entries of 256 KiB, 1, 4, 16 and 64 MiB, option on (threshold 1) against option off: the crossover;
  (E) option 0 on the archive of (C) against the library at --parent-lib (the parent commit's build), through ctypes on
      the same card: the path is unchanged, so the two must lie inside the pair's own spread.
Every archive is put on the device and timed with device pointers, whole calls, best of --reps, the two calls of a pair
ALTERNATED on the same card (a, b, a, b, ...; the first call of each sizes the ctx's scratch and is not counted); the
output of every option-on read is compared with the input once.  Prints one JSON line; also written to $FLATE_OUT_ROOT
(default results/)/zip_units_bench.json."""
import argparse
import ctypes as C
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
from gzfile_bench import HEADER  # noqa: E402
from one_bench import workload  # noqa: E402


def raw_streams(plain, n, level):
    """plain as n raw DEFLATE streams of equal size -> [(raw, crc, size)] (zlib releases the GIL)."""
    size = plain.size // n

    def one(k):
        p = plain[k * size:(k + 1) * size].tobytes()
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        return co.compress(p) + co.flush(), zlib.crc32(p), len(p)

    with ThreadPoolExecutor(max_workers=16) as pool:
        return list(pool.map(one, range(n), chunksize=max(1, n // 64)))


def archive(streams):
    """The ZIP archive of these streams, entry k named e<k>."""
    parts, central, at = [], [], 0
    for k, (raw, crc, size) in enumerate(streams):
        name = b"e%d" % k
        parts.append(struct.pack("<4sHHHHHIIIHH", b"PK\3\4", 20, 0x0800, 8, 0, 0x0021, crc, len(raw), size, len(name), 0) + name)
        parts.append(raw)
        central.append(struct.pack("<4sHHHHHHIIIHHHHHII", b"PK\1\2", 20, 20, 0x0800, 8, 0, 0x0021, crc, len(raw), size,
                                   len(name), 0, 0, 0, 0, 0, at) + name)
        at += 30 + len(name) + len(raw)
    cd = b"".join(central)
    assert at + len(cd) < 0xffffffff and len(streams) < 65535
    return b"".join(parts) + cd + struct.pack("<4sHHHHIIH", b"PK\5\6", 0, 0, len(streams), len(streams), len(cd), at, 0)


def gzip_file(streams):
    return b"".join(HEADER + raw + struct.pack("<II", crc, size & 0xffffffff) for raw, crc, size in streams)


def raw_zip_read(L, ctx, d, n, out, cap):
    """ONE flate_hip_zip_read call over every entry (sel == NULL), device pointers -> (rc, bytes, entries)."""
    ooff, olen = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    st, eo = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int64)
    ne, aeo = C.c_uint32(0), C.c_int64(-1)
    rc = L.flate_hip_zip_read(ctx, d.data_ptr(), d.numel(), None, 0, n, out.data_ptr(), cap, ooff.ctypes.data,
                              olen.ctypes.data, st.ctypes.data, eo.ctypes.data, C.byref(ne), C.byref(aeo), 1)
    return rc, int(ooff[n]), int(ne.value)


class ParentLib:
    """flate_hip_zip_read of another build of the library, through ctypes alone."""

    def __init__(self, path):
        self.L = C.CDLL(path)
        self.L.flate_hip_init.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        self.L.flate_hip_zip_read.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32,
                                              C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_uint32]
        self.L.flate_hip_build_id.restype = C.c_char_p
        self.L.flate_hip_destroy.argtypes = [C.c_void_p]
        self.ctx = C.c_void_p()
        assert self.L.flate_hip_init(0, C.byref(self.ctx)) == 0
        self.build_id = self.L.flate_hip_build_id().decode()

    def zip_read(self, d, n, out, cap):
        return raw_zip_read(self.L, self.ctx, d, n, out, cap)

    def close(self):
        self.L.flate_hip_destroy(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="ABCDE")
    ap.add_argument("--parent-lib", default="")
    a = ap.parse_args()
    import torch

    plain = workload("text", a.mib)
    eng = flate.FlateEngine(0)
    out = torch.empty(plain.size + 16, dtype=torch.uint8, device="cuda")
    want = torch.from_numpy(plain)
    res = {"what": "ZIP archives of one S-text, device pointers, whole calls, ms, pairs alternated",
           "plain_bytes": int(plain.size), "zlib_level": a.level, "reps": a.reps, "build_id": flate.build_id()}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()  # (every call ends with a read-back of its result words behind a synchronise)
        return r, (time.perf_counter() - t0) * 1e3

    def device(b):
        return torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()

    def zread(d, unit_min, n):
        eng.set_option("zip_unit_min", unit_min)
        r = raw_zip_read(eng._L, eng._ctx, d, n, out, plain.size)
        return r, eng.zip_last_route()

    def pair(ours, theirs, check):
        """best-of times of two calls alternated; check(result of ours, rep)"""
        t_a, t_b = [], []
        for rep in range(a.reps + 1):
            r, t = timed(ours)
            check(r, rep)
            t_a.append(round(t, 3))
            if theirs:
                q, t = timed(theirs)
                t_b.append(round(t, 3))
        return t_a, t_b

    def zip_check(n_bytes, n_entries, served):
        def check(r, rep):
            zr, route = r
            assert zr == (0, n_bytes, n_entries), zr
            assert served is None or route[0] == served, route
            if rep == 0:
                assert bool((out[:n_bytes].cpu() == want[:n_bytes]).all()), "the output is not the input"
        return check

    def best(ts):
        return min(ts[1:])

    def gibps(n_bytes, ms):
        return round(n_bytes / 2**30 / (ms * 1e-3), 3)

    sized = {}

    def streams_of(n):
        if n not in sized:
            t0 = time.perf_counter()
            sized[n] = raw_streams(plain, n, a.level)
            print("%d streams compressed in %.1f s" % (n, time.perf_counter() - t0), file=sys.stderr, flush=True)
        return sized[n]

    for key in a.only:
        if key == "A":
            s = streams_of(1)
            d, d_raw = device(archive(s)), device(s[0][0])
            t_on, t_one = pair(lambda: zread(d, 1, 1), lambda: eng.inflate_one(d_raw, "raw", out=out)[1],
                               zip_check(plain.size, 1, 1))
            route = eng.zip_last_route()
            small = plain[:64 << 20]
            s64 = raw_streams(small, 1, a.level)
            d64 = device(archive(s64))
            t_off64, t_on64 = pair(lambda: zread(d64, 0, 1), lambda: zread(d64, 1, 1), zip_check(small.size, 1, 0))
            row = {"entries": 1, "n_units": route[2], "n_candidates": route[3], "on_ms_best": best(t_on), "on_ms_all": t_on,
                   "on_gib_per_s": gibps(plain.size, best(t_on)), "against": "inflate_one (raw)",
                   "against_ms_best": best(t_one), "against_ms_all": t_one, "ratio": round(best(t_on) / best(t_one), 3),
                   "one_entry_of_64_mib": {"off_ms_best": best(t_off64), "off_ms_all": t_off64, "on_ms_best": best(t_on64),
                                           "on_ms_all": t_on64, "off_mib_per_s": round(64 / (best(t_off64) * 1e-3), 1)}}
            del d, d_raw, d64
            sized.pop(1, None)
        elif key == "B":
            s = streams_of(16)
            d, dg = device(archive(s)), device(gzip_file(s))
            t_on, t_gz = pair(lambda: zread(d, 1, 16), lambda: eng.gzfile_read(dg, out=out)[1], zip_check(plain.size, 16, 16))
            route = eng.zip_last_route()
            row = {"entries": 16, "n_units": route[2], "on_ms_best": best(t_on), "on_ms_all": t_on,
                   "on_gib_per_s": gibps(plain.size, best(t_on)), "against": "gzfile_read", "against_ms_best": best(t_gz),
                   "against_ms_all": t_gz, "ratio": round(best(t_on) / best(t_gz), 3)}
            del d, dg
        elif key in "CE":
            n = a.mib * 16
            s = streams_of(n)
            d = device(archive(s))
            if key == "C":
                t_on, t_off = pair(lambda: zread(d, 1, n), lambda: zread(d, 0, n), zip_check(plain.size, n, n))
                route = eng.zip_last_route()
                row = {"entries": n, "n_units": zread(d, 1, n)[1][2], "on_ms_best": best(t_on), "on_ms_all": t_on,
                       "off_ms_best": best(t_off), "off_ms_all": t_off, "ratio": round(best(t_on) / best(t_off), 3)}
            else:
                assert a.parent_lib, "(E) needs --parent-lib"
                par = ParentLib(a.parent_lib)

                def theirs():
                    assert par.zip_read(d, n, out, plain.size) == (0, plain.size, n)

                t_off, t_par = pair(lambda: zread(d, 0, n), theirs, zip_check(plain.size, n, 0))
                row = {"entries": n, "off_ms_best": best(t_off), "off_ms_all": t_off, "parent_build_id": par.build_id,
                       "parent_ms_best": best(t_par), "parent_ms_all": t_par,
                       "spread_ms": {"this": round(max(t_off[1:]) - min(t_off[1:]), 3),
                                     "parent": round(max(t_par[1:]) - min(t_par[1:]), 3)}}
                par.close()
            del d
        elif key == "D":
            row = {}
            for kib in (256, 1024, 4096, 16384, 65536):
                n = a.mib * 1024 // kib
                s = streams_of(n)
                d = device(archive(s))
                t_on, t_off = pair(lambda: zread(d, 1, n), lambda: zread(d, 0, n), zip_check(plain.size, n, n))
                row["%d KiB" % kib] = {"entries": n, "on_ms_best": best(t_on), "on_ms_all": t_on, "off_ms_best": best(t_off),
                                       "off_ms_all": t_off, "ratio": round(best(t_on) / best(t_off), 3)}
                print(json.dumps({kib: row["%d KiB" % kib]}), file=sys.stderr, flush=True)
                del d
                if n not in (16, a.mib * 16):
                    sized.pop(n, None)
        else:
            continue
        res[key] = row
        print(json.dumps({key: row}), file=sys.stderr, flush=True)
    eng.close()
    line = json.dumps(res)
    print(line)
    out_root = os.environ.get("FLATE_OUT_ROOT", os.path.join(ROOT, "results"))
    os.makedirs(out_root, exist_ok=True)
    with open(os.path.join(out_root, "zip_units_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
