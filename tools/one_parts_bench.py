#!/usr/bin/env python3
"""One long gzip member read in PARTS (flate_hip_one_reader_*) against the whole call (flate_hip_inflate_one).

    python tools/one_parts_bench.py [--mib 1024] [--level 6] [--reps 5] [--parts 16,64,256] [--member FILE] [--save FILE]
                                    [--whole-only]

The input is --mib MiB of S-text as ONE gzip member compressed with zlib at --level (on the CPU, once; --save keeps it,
--member loads a kept one), resident on the device.  A PASS reads the whole member through the reader in parts of P MiB
of compressed bytes (a part begins where the last call's in_used ends: a slice of the resident stream, nothing is
moved) into one output buffer of 4 P MiB, with device pointers.  Per P: best of --reps passes, each ALTERNATED in this
process with one flate_hip_inflate_one on the whole file; calls per pass; units discovered twice (units that start
inside a call's part and are not delivered by it -- the cut unit and those that did not fit --, from the whole call's
index).  One pass with host pointers and 64 MiB parts, and flate_hip_inflate_stream_read on the first 2 MiB of the
member for its rate.  `spread` is the largest difference between two calls of the same kind.  --whole-only: the whole
call alone, --reps + 1 times (for a comparison between two builds of the library, FLATE_HIP_LIB).  Prints one JSON
line; also written to $FLATE_OUT_ROOT (default results/)/one_parts_bench.json."""
import argparse
import importlib
import json
import os
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
flate = importlib.import_module("moonbit-flate_amd")
MIB = 1 << 20


def make_member(mib, level):
    plain = flate.synth("text", mib * 16, 65536)
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    raw = c.compress(plain.tobytes()) + c.flush()
    return flate.engine.GZIP_HEADER + raw + struct.pack("<II", zlib.crc32(plain), plain.size & 0xffffffff), int(plain.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", default="16,64,256")
    ap.add_argument("--member")
    ap.add_argument("--save")
    ap.add_argument("--whole-only", action="store_true")
    a = ap.parse_args()
    import torch

    t0 = time.perf_counter()
    if a.member:
        f = open(a.member, "rb").read()
        T = struct.unpack("<I", f[-4:])[0] or 1 << 32
    else:
        f, T = make_member(a.mib, a.level)
        if a.save:
            open(a.save, "wb").write(f)
    print("%d bytes -> %d, ready in %.1f s" % (T, len(f), time.perf_counter() - t0), file=sys.stderr, flush=True)
    h = np.frombuffer(f, np.uint8)
    d = torch.from_numpy(h.copy()).cuda()
    eng = flate.FlateEngine(0)
    whole_out = torch.empty(T + 16, dtype=torch.uint8, device="cuda")
    res = {"what": "one gzip member of S-text, whole passes, ms", "plain_bytes": T, "file_bytes": len(f),
           "zlib_level": a.level, "reps": a.reps, "build_id": flate.build_id()}

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, round((time.perf_counter() - t) * 1e3, 3)

    def whole():
        _, q = eng.inflate_one(d, "gzip", out=whole_out)
        assert q.rc == 0 and q.out_len == T, q
        return q

    def spread(t):
        return round(max(t[1:]) - min(t[1:]), 3)

    if a.whole_only:
        times = [timed(whole)[1] for _ in range(a.reps + 1)]
        res["whole_ms_all"], res["whole_ms_best"], res["whole_spread_ms"] = times, min(times[1:]), spread(times)
        print(json.dumps(res))
        return
    q = whole()
    ix = eng.inflate_one_index(d, "gzip")
    unit_byte = 10 + (np.asarray(ix.unit_bit[:-1], dtype=np.uint64) >> np.uint64(3)).astype(np.int64)  # in the member
    res["n_units"], res["n_candidates"] = q.n_units, q.n_candidates

    def a_pass(data, part, out, check):
        """The whole member through the reader -> (calls, units discovered twice)."""
        rd = eng.open_one_reader("gzip", device=flate.engine._is_torch(data))
        pos, calls, twice, total = 0, 0, 0, 0
        n = len(f)
        while True:
            end = min(pos + part, n)
            used, got, r = rd.read(data[pos:end], final=end == n, out=out)
            calls += 1
            assert r.rc in (0, 1) and (used or r.out_len), (r, pos)  # (a part holds many units: every call moves)
            twice += int(np.searchsorted(unit_byte, end) - np.searchsorted(unit_byte, pos)) - r.n_units
            if check and calls == 2:
                assert bool((got == whole_out[total:total + r.out_len]).all())
            total += r.out_len
            pos += used
            if r.rc == 1:
                break
        rd.close()
        assert total == T and pos == n, (total, pos)
        return calls, twice

    for p in [int(x) for x in a.parts.split(",")]:
        part = p * MIB
        out = torch.empty(4 * part, dtype=torch.uint8, device="cuda")
        tp, tw = [], []
        for rep in range(a.reps + 1):  # (the first pair sizes the scratch)
            (calls, twice), t = timed(lambda: a_pass(d, part, out, rep == 0))
            tp.append(t)
            tw.append(timed(whole)[1])
        res["parts_%d_mib" % p] = {"pass_ms_best": min(tp[1:]), "pass_ms_all": tp, "pass_spread_ms": spread(tp),
                                   "whole_ms_best": min(tw[1:]), "whole_ms_all": tw, "whole_spread_ms": spread(tw),
                                   "calls": calls, "units_discovered_twice": twice,
                                   "out_mb_per_s": round(T / 1e6 / (min(tp[1:]) / 1e3), 1)}
        print(json.dumps({p: res["parts_%d_mib" % p]}), file=sys.stderr, flush=True)
        del out
    out = np.zeros(4 * 64 * MIB, np.uint8)
    (calls, twice), t = timed(lambda: a_pass(h, 64 * MIB, out, False))
    res["host_pointers_64_mib"] = {"pass_ms": t, "calls": calls, "out_mb_per_s": round(T / 1e6 / (t / 1e3), 1)}
    sr = eng.open_inflate_stream()
    (got, rc), t = timed(lambda: sr.feed(h[10:10 + 2 * MIB], final=False, room=64 * MIB))
    res["inflate_stream_read_2_mib"] = {"ms": t, "out_bytes": int(got.size), "out_mb_per_s": round(got.size / 1e6 / (t / 1e3), 2)}
    sr.free()
    eng.close()
    line = json.dumps(res)
    print(line)
    out_root = os.environ.get("FLATE_OUT_ROOT", os.path.join(ROOT, "results"))
    os.makedirs(out_root, exist_ok=True)
    with open(os.path.join(out_root, "one_parts_bench.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
