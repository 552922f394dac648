#!/usr/bin/env python3
"""A gzip FILE of any members read in PARTS (flate_hip_gzfile_reader_*) against the calls a caller has without it.

    python tools/gzfile_parts_bench.py [--mib 1024] [--level 6] [--reps 5] [--parts 16,64,256] [--only A,B,C]
                                       [--whole-only] [--cache DIR]

The input is --mib MiB of S-text compressed with zlib at --level (on the CPU, once per workload, the members in
parallel), resident on the device, as
  A  ONE member                      parts of --parts MiB; against flate_hip_one_reader_read with the same parts and
                                     flate_hip_gzfile_read whole
  B  16 members of --mib / 16 MiB    the same parts; against flate_hip_gzfile_read whole and THE LOOP a caller must
                                     write today: the one reader, reset at every member's end
  C  members of 64 KiB               parts of 64 MiB; against that loop (it is a call per member: its first 256 calls
                                     are timed once and the pass is extrapolated from them), flate_hip_gzfile_read
                                     whole and flate_hip_gzip_read
A PASS reads the whole file through the reader in parts of P MiB of compressed bytes (a part begins where the last
call's in_used ends: a slice of the resident file, nothing is moved) into one output buffer of 4 P MiB, with device
pointers.  Per P: best of --reps passes, each ALTERNATED in this process with its comparison call on the same card;
`spread` is the largest difference between two calls of the same kind.  --whole-only: flate_hip_gzfile_read and
flate_hip_one_reader_read (64 MiB parts) on workload A alone, --reps + 1 times each (for a comparison between two
builds of the library, FLATE_HIP_LIB; --cache DIR keeps the compressed files between such runs).  Host pointers and
per-step times are not measured.  Prints one JSON line; also written to $FLATE_OUT_ROOT (default results/)/gzfile_parts_bench.json."""
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
    """The file of members of member_bytes plain bytes each -> (file, the members' offsets)."""
    cuts = list(range(0, len(plain), member_bytes))
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:  # (zlib releases the interpreter's lock)
        ms = list(ex.map(lambda a: member(plain[a:a + member_bytes], level), cuts))
    off = np.concatenate([[0], np.cumsum([len(m) for m in ms])]).astype(np.int64)
    return b"".join(ms), off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", default="16,64,256")
    ap.add_argument("--only", default="A,B,C")
    ap.add_argument("--whole-only", action="store_true")
    ap.add_argument("--cache")
    a = ap.parse_args()
    import torch

    plain = memoryview(flate.synth("text", a.mib * 16, 65536).tobytes())
    T = len(plain)
    eng = flate.FlateEngine(0)
    whole_out = torch.empty(T + 16, dtype=torch.uint8, device="cuda")
    res = {"what": "gzip files of S-text, whole passes, ms, device pointers", "plain_bytes": T, "zlib_level": a.level,
           "reps": a.reps, "build_id": flate.build_id(), "not_measured": ["host pointers", "per-step times"]}

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, round((time.perf_counter() - t) * 1e3, 3)

    def spread(t):
        return round(max(t[1:]) - min(t[1:]), 3) if len(t) > 2 else 0.0

    def stats(t):
        return {"ms_best": min(t[1:]) if len(t) > 1 else t[0], "ms_all": t, "spread_ms": spread(t)}

    def gz_pass(d, n, part, out, check):
        """The whole file through the gzip file reader -> (calls, members)."""
        rd = eng.open_gzfile_reader(device=True)
        pos, calls, total, members = 0, 0, 0, 0
        while True:
            end = min(pos + part, n)
            used, got, r = rd.read(d[pos:end], final=end == n, out=out)
            calls += 1
            assert r.rc in (0, 1) and (used or r.out_len), (r, pos)
            if check and calls == 2:
                assert bool((got == whole_out[total:total + r.out_len]).all())
            total, pos, members = total + r.out_len, pos + used, members + r.n_members
            if r.rc == 1:
                break
        rd.close()
        assert total == T and pos == n, (total, pos)
        return calls, members

    def one_pass(d, n, part, out, limit=None):
        """THE LOOP of today: the one reader, reset at every member's end -> calls (limit: the first calls only)."""
        rd = eng.open_one_reader("gzip", device=True)
        pos, calls, total = 0, 0, 0
        while pos < n and (limit is None or calls < limit):
            end = min(pos + part, n)
            used, got, r = rd.read(d[pos:end], final=False, out=out)
            calls += 1
            assert r.rc in (0, 1) and (used or r.out_len), (r, pos)
            total, pos = total + r.out_len, pos + used
            if r.rc == 1:
                rd.reset()
        rd.close()
        assert total == T or limit is not None, total
        return calls

    def whole(d):
        _, q = eng.gzfile_read(d, out=whole_out)
        assert q.rc == 0 and q.out_len == T, q
        return q

    parts = [int(x) for x in a.parts.split(",")]
    for name in a.only.split(","):
        t0 = time.perf_counter()
        mb = {"A": T, "B": max(T // 16, 65536), "C": 65536}[name]
        kept = os.path.join(a.cache, "%s_%d_%d" % (name, a.mib, a.level)) if a.cache else None
        if kept and os.path.exists(kept + ".gz"):
            f, off = open(kept + ".gz", "rb").read(), np.load(kept + ".npy")
        else:
            f, off = make_file(plain, mb, a.level)
            if kept:
                os.makedirs(a.cache, exist_ok=True)
                open(kept + ".gz", "wb").write(f)
                np.save(kept + ".npy", off)
        n = len(f)
        d = torch.from_numpy(np.frombuffer(f, np.uint8).copy()).cuda()
        print("%s: %d members, %d bytes, ready in %.1f s" % (name, len(off) - 1, n, time.perf_counter() - t0), file=sys.stderr, flush=True)
        w = res[name] = {"members": len(off) - 1, "file_bytes": n}
        if a.whole_only:
            if name == "A":
                out = torch.empty(4 * 64 * MIB, dtype=torch.uint8, device="cuda")
                tw, to = [], []
                for _ in range(a.reps + 1):
                    tw.append(timed(lambda: whole(d))[1])
                    to.append(timed(lambda: one_pass(d, n, 64 * MIB, out))[1])
                w["gzfile_read"], w["one_reader_64_mib"] = stats(tw), stats(to)
            continue
        q = whole(d)
        w["n_units"] = q.n_units
        for p in (parts if name != "C" else [64]):
            part = p * MIB
            out = torch.empty(4 * part, dtype=torch.uint8, device="cuda")
            tp, tw, to = [], [], []
            # (C: a call per member, each with FIND over the whole part -- the first 256 calls, once, and the pass
            # extrapolated from them)
            loop_reps, limit = (a.reps, None) if name != "C" else (0, 256)
            for rep in range(a.reps + 1):  # (the first round sizes the scratch)
                (calls, members), t = timed(lambda: gz_pass(d, n, part, out, rep == 0))
                tp.append(t)
                tw.append(timed(lambda: whole(d))[1])
                if rep <= loop_reps:
                    one_calls, t = timed(lambda: one_pass(d, n, part, out, limit))
                    to.append(t)
            assert members == len(off) - 1
            w["parts_%d_mib" % p] = {"reader": stats(tp), "calls": calls, "gzfile_read": stats(tw),
                                     "one_reader" + ("" if name == "A" else "_reset_per_member"): stats(to),
                                     "one_reader_calls": one_calls,
                                     "out_mb_per_s": round(T / 1e6 / (stats(tp)["ms_best"] / 1e3), 1)}
            if limit:
                w["parts_%d_mib" % p]["one_reader_pass_ms_extrapolated"] = round(to[0] * (len(off) - 1) / one_calls, 1)
            print(json.dumps({name: {p: w["parts_%d_mib" % p]}}), file=sys.stderr, flush=True)
            del out
        if name == "C":
            tg = []
            for _ in range(a.reps + 1):
                _, t = timed(lambda: eng.gzip_read(d, out=whole_out))
                tg.append(t)
            w["gzip_read"] = stats(tg)
        del d
    eng.close()
    line = json.dumps(res)
    print(line)
    out_root = os.environ.get("FLATE_OUT_ROOT", os.path.join(ROOT, "results"))
    os.makedirs(out_root, exist_ok=True)
    with open(os.path.join(out_root, "gzfile_parts_bench.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
