#!/usr/bin/env python3
"""The seek index of a gzip file of any members: flate_hip_gzfile_seek_index and flate_hip_gzfile_ranges against the
call each kind of file had before.

    python tools/gzfile_seek_bench.py [--mib 1024] [--level 6] [--reps 5] [--only ABC]

The input is tools/gzfile_bench.py's: --mib MiB of S-text compressed with zlib at --level (on the CPU, once) into
  (A) ONE gzip member, span 1 MiB: the build against flate_hip_inflate_one_seek_index, 4096 random ranges of 64 KiB
      against flate_hip_inflate_one_ranges -- the kernels are the same, so the expectation is "inside each other's
      spread";
  (B) 16 members of --mib / 16 MiB, span 1 MiB: the build against flate_hip_gzfile_read; [0, T); 4096 random ranges of
      64 KiB; one range of 1 byte;
  (C) --mib * 16 members of 64 KiB, span NONE: the build; one range of 1 byte; 4096 random ranges of 64 KiB against
      flate_hip_gzip_read of the whole file.
Every file is on the device; whole calls with device pointers, best of --reps after one call that sizes the ctx's
scratch, the two calls of a pair ALTERNATED on the same card.  `spread` is the largest difference between two calls of
the same kind inside a pair's lists: a difference between the kinds below it says nothing.  Index and window sizes are
recorded per file.  Prints one JSON line; also written to $FLATE_OUT_ROOT (default results/)/gzfile_seek_bench.json."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
flate = importlib.import_module("moonbit-flate_amd")
import gzfile_bench  # noqa: E402  (make: the same files)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="ABC")
    a = ap.parse_args()
    import torch

    plain = flate.synth("text", a.mib * 16, 65536)
    T = int(plain.size)
    counts = {"A": 1, "B": 16, "C": a.mib * 16}
    spans = {"A": 1 << 20, "B": 1 << 20, "C": flate.SEEK_SPAN_NONE}
    eng = flate.FlateEngine(0)
    out = torch.empty(T + 16, dtype=torch.uint8, device="cuda")
    d_plain = torch.from_numpy(plain).cuda()
    rng = np.random.default_rng(5)
    begin = rng.integers(0, max(T - 65536, 1), 4096).astype(np.uint64)
    end = np.minimum(begin + np.uint64(65536), np.uint64(T))
    at = T // 2 + 12345
    res = {"what": "gzip files of one S-text, device pointers, whole calls, ms, pairs alternated", "plain_bytes": T,
           "zlib_level": a.level, "reps": a.reps, "build_id": flate.build_id()}

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

    def check_ranges(o, rr):
        assert rr.rc == 0 and int(rr.out_off[-1]) == int((end - begin).sum()), rr
        for r in (0, 1, 4095):
            assert bool((o[int(rr.out_off[r]):int(rr.out_off[r + 1])] == d_plain[int(begin[r]):int(end[r])]).all()), r

    for key in a.only:
        t0 = time.perf_counter()
        f = gzfile_bench.make(plain, counts[key], a.level)
        d = torch.from_numpy(np.frombuffer(f, np.uint8).copy()).cuda()
        print("%s: %d members, %d bytes, compressed in %.1f s" % (key, counts[key], len(f), time.perf_counter() - t0),
              file=sys.stderr, flush=True)
        span = spans[key]
        build = lambda: eng.gzfile_seek_index(d, span)
        ranges = lambda s: eng.gzfile_ranges(d, s, begin, end, out=out)
        row = {"members": counts[key], "file_bytes": len(f), "span": "none" if span == flate.SEEK_SPAN_NONE else span}
        if key == "A":
            s, s1, t_build, t_theirs = alternated(build, lambda: eng.inflate_one_seek_index(d, "gzip", span))
            assert s.rc == 0 and s1.rc == 0 and (s.n_units, s.n_points) == (s1.n_units, s1.n_points), (s.rc, s1.rc)
            row.update({"build_ms_best": min(t_build[1:]), "build_ms_all": t_build, "build_against": "inflate_one_seek_index",
                        "build_against_ms_best": min(t_theirs[1:]), "build_against_ms_all": t_theirs,
                        "build_spread_ms": spread(t_build, t_theirs)})
            (o, rr), (_, r1), t_rand, t_theirs = alternated(lambda: ranges(s),
                                                            lambda: eng.inflate_one_ranges(d, s1, begin, end, out=out))
            assert r1.rc == 0
            (o, rr) = ranges(s)
            check_ranges(o, rr)
            row.update({"ranges_4096x64k_ms_best": min(t_rand[1:]), "ranges_4096x64k_ms_all": t_rand,
                        "ranges_against": "inflate_one_ranges", "ranges_against_ms_best": min(t_theirs[1:]),
                        "ranges_against_ms_all": t_theirs, "ranges_spread_ms": spread(t_rand, t_theirs),
                        "ranges_n_decoded": rr.n_decoded})
        elif key == "B":
            s, (_, rd), t_build, t_theirs = alternated(build, lambda: eng.gzfile_read(d, out=out))
            assert s.rc == 0 and rd.rc == 0 and rd.out_len == T, (s.rc, rd)
            row.update({"build_ms_best": min(t_build[1:]), "build_ms_all": t_build, "build_against": "gzfile_read",
                        "build_against_ms_best": min(t_theirs[1:]), "build_against_ms_all": t_theirs,
                        "build_spread_ms": spread(t_build, t_theirs)})
            (o, rw), t_whole = best(lambda: eng.gzfile_ranges(d, s, [0], [T], out=out))
            assert rw.rc == 0 and int(rw.out_off[1]) == T and bool((o[:T] == d_plain).all()), rw
            (o, rr), t_rand = best(lambda: ranges(s))
            check_ranges(o, rr)
            (o, rb), t_byte = best(lambda: eng.gzfile_ranges(d, s, [at], [at + 1], out=out))
            assert rb.rc == 0 and int(o[0]) == int(plain[at])
            row.update({"whole_ms_best": min(t_whole[1:]), "whole_ms_all": t_whole, "whole_n_decoded": rw.n_decoded,
                        "ranges_4096x64k_ms_best": min(t_rand[1:]), "ranges_4096x64k_ms_all": t_rand,
                        "ranges_n_decoded": rr.n_decoded, "one_byte_ms_best": min(t_byte[1:]), "one_byte_ms_all": t_byte,
                        "one_byte_n_decoded": rb.n_decoded})
        else:
            s, t_build = best(build)
            assert s.rc == 0, s.rc
            (o, rb), t_byte = best(lambda: eng.gzfile_ranges(d, s, [at], [at + 1], out=out))
            assert rb.rc == 0 and int(o[0]) == int(plain[at])
            (o, rr), (_, rg), t_rand, t_theirs = alternated(lambda: ranges(s), lambda: eng.gzip_read(d, out=out))
            assert rg.rc == 0 and rg.out_len == T, rg
            (o, rr) = ranges(s)
            check_ranges(o, rr)
            row.update({"build_ms_best": min(t_build[1:]), "build_ms_all": t_build, "one_byte_ms_best": min(t_byte[1:]),
                        "one_byte_ms_all": t_byte, "one_byte_n_decoded": rb.n_decoded,
                        "ranges_4096x64k_ms_best": min(t_rand[1:]), "ranges_4096x64k_ms_all": t_rand,
                        "ranges_n_decoded": rr.n_decoded, "ranges_against": "gzip_read of the whole file",
                        "ranges_against_ms_best": min(t_theirs[1:]), "ranges_against_ms_all": t_theirs,
                        "ranges_spread_ms": spread(t_rand, t_theirs)})
        row.update({"n_units": s.n_units, "n_points": s.n_points, "index_bytes": int(s.index.size) * 8,
                    "windows_bytes": int(s.windows.numel())})
        res[key] = row
        print(json.dumps({key: row}), file=sys.stderr, flush=True)
        del d, s
    eng.close()
    line = json.dumps(res)
    print(line)
    out_root = os.environ.get("FLATE_OUT_ROOT", os.path.join(ROOT, "results"))
    os.makedirs(out_root, exist_ok=True)
    with open(os.path.join(out_root, "gzfile_seek_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
