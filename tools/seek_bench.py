#!/usr/bin/env python3
"""The seek index of one long gzip member: flate_hip_inflate_one_seek_index and flate_hip_inflate_one_ranges against
flate_hip_inflate_one on the same file.

    python tools/seek_bench.py [--mib 1024] [--level 6] [--reps 5] [--workload text|random|mixed] [--stored-units]

The input is tools/one_bench.py's: --mib MiB of S-text compressed with zlib at --level into ONE gzip member (on the
CPU, once), on the device; whole calls with device pointers, best of --reps after one call that sizes the ctx's scratch.
  (a) the build at span 1 MiB, ALTERNATED with flate_hip_inflate_one pair by pair on the same card
  (b) [0, T) through an index without points (FLATE_HIP_SEEK_SPAN_NONE), alternated with flate_hip_inflate_one
  (c) 4096 random ranges of 64 KiB through the 1 MiB index
  (d) one range of 1 byte through the 1 MiB index       (e) the same byte through an index of span 64 KiB
and the index and window sizes of every span.  `spread` is the largest difference between two calls of the same kind
inside the alternated pairs: a difference between the kinds below it says nothing.  Prints one JSON line; also written
to $FLATE_OUT_ROOT (default results/)/seek_bench.json.  --workload and --stored-units are tools/one_bench.py's: other
plain bytes, and the option "one_stored_units" on the building ctx (a read takes the rule from the index); with the
mixed workload the one byte of (d) and (e) lies in the middle of a random stretch."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
flate = importlib.import_module("moonbit-flate_amd")
from one_bench import workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workload", choices=("text", "random", "mixed"), default="text")
    ap.add_argument("--stored-units", action="store_true")
    a = ap.parse_args()
    import torch

    plain = workload(a.workload, a.mib)
    co = zlib.compressobj(a.level, zlib.DEFLATED, -15)
    raw = co.compress(plain.tobytes()) + co.flush()
    member = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + raw + struct.pack("<II", zlib.crc32(plain), plain.size & 0xffffffff)
    T = int(plain.size)
    eng = flate.FlateEngine(0)
    eng.set_option("one_stored_units", 1 if a.stored_units else 0)
    d = torch.from_numpy(np.frombuffer(member, np.uint8).copy()).cuda()
    out = torch.empty(T + 16, dtype=torch.uint8, device="cuda")
    d_plain = torch.from_numpy(plain).cuda()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, round((time.perf_counter() - t0) * 1e3, 3)

    def alternated(fa, fb):
        """reps + 1 pairs (a, b); the first pair sizes the scratch -> (last results, times of a, times of b)."""
        ta, tb = [], []
        for _ in range(a.reps + 1):
            ra, t = timed(fa)
            ta.append(t)
            rb, t = timed(fb)
            tb.append(t)
        return ra, rb, ta, tb

    def best(fn):
        times = []
        for _ in range(a.reps + 1):
            r, t = timed(fn)
            times.append(t)
        return r, times

    def spread(*lists):
        return round(max(max(t[1:]) - min(t[1:]) for t in lists), 3)

    one = lambda: eng.inflate_one(d, "gzip", out=out)
    # (a)
    s_mib, (_, rd), t_build, t_one_a = alternated(lambda: eng.inflate_one_seek_index(d, "gzip", 1 << 20), one)
    assert s_mib.rc == 0 and rd.rc == 0 and rd.out_len == T, (s_mib.rc, rd)
    # (b)
    s_none = eng.inflate_one_seek_index(d, "gzip", flate.SEEK_SPAN_NONE)
    whole = lambda: eng.inflate_one_ranges(d, s_none, [0], [T], out=out)
    (_, rw), _, t_whole, t_one_b = alternated(whole, one)
    assert rw.rc == 0 and int(rw.out_off[1]) == T, rw
    whole()
    assert bool((out[:T] == d_plain).all()), "[0, T) through the index is not the input"
    # (c)
    rng = np.random.default_rng(5)
    begin = rng.integers(0, max(T - 65536, 1), 4096).astype(np.uint64)
    end = np.minimum(begin + np.uint64(65536), np.uint64(T))
    (o, rr), t_rand = best(lambda: eng.inflate_one_ranges(d, s_mib, begin, end, out=out))
    assert rr.rc == 0 and int(rr.out_off[-1]) == int((end - begin).sum()), rr
    for r in (0, 1, 4095):
        assert bool((o[int(rr.out_off[r]):int(rr.out_off[r + 1])] == d_plain[int(begin[r]):int(end[r])]).all()), r
    # (d), (e)
    at = T // 2 + 12345
    if a.workload == "mixed" and (at >> 20) % 2 == 0 and at + (1 << 20) < T:
        at += 1 << 20  # (the even MiB rows are text, the odd ones random bytes: tools/one_bench.py workload)
    (o, r1), t_byte_mib = best(lambda: eng.inflate_one_ranges(d, s_mib, [at], [at + 1], out=out))
    assert r1.rc == 0 and int(o[0]) == int(plain[at])
    s_64k = eng.inflate_one_seek_index(d, "gzip", 65536)
    (o, r2), t_byte_64k = best(lambda: eng.inflate_one_ranges(d, s_64k, [at], [at + 1], out=out))
    assert r2.rc == 0 and int(o[0]) == int(plain[at])

    def sizes(s):
        return {"index_bytes": int(s.index.size) * 8, "windows_bytes": int(s.windows.numel()), "n_points": s.n_points}

    res = {
        "what": "one gzip member, device pointers, whole calls, ms",
        "workload": a.workload, "one_stored_units": int(a.stored_units), "n_candidates": rd.n_candidates,
        "plain_bytes": T, "member_bytes": len(member), "zlib_level": a.level, "n_units": s_mib.n_units,
        "a_build_1mib_ms_best": min(t_build[1:]), "a_build_1mib_ms_all": t_build,
        "a_inflate_one_ms_best": min(t_one_a[1:]), "a_inflate_one_ms_all": t_one_a, "a_spread_ms": spread(t_build, t_one_a),
        "b_whole_span_none_ms_best": min(t_whole[1:]), "b_whole_span_none_ms_all": t_whole,
        "b_inflate_one_ms_best": min(t_one_b[1:]), "b_inflate_one_ms_all": t_one_b, "b_spread_ms": spread(t_whole, t_one_b),
        "c_4096_ranges_64k_ms_best": min(t_rand[1:]), "c_4096_ranges_64k_ms_all": t_rand, "c_n_decoded": rr.n_decoded,
        "d_one_byte_1mib_ms_best": min(t_byte_mib[1:]), "d_one_byte_1mib_ms_all": t_byte_mib, "d_n_decoded": r1.n_decoded,
        "e_one_byte_64k_ms_best": min(t_byte_64k[1:]), "e_one_byte_64k_ms_all": t_byte_64k, "e_n_decoded": r2.n_decoded,
        "span_1mib": sizes(s_mib), "span_64k": sizes(s_64k), "span_none": sizes(s_none),
        "build_id": flate.build_id(),
    }
    line = json.dumps(res)
    print(line)
    out_root = os.environ.get("FLATE_OUT_ROOT", os.path.join(ROOT, "results"))
    os.makedirs(out_root, exist_ok=True)
    with open(os.path.join(out_root, "seek_bench.json"), "w") as f:
        f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
