#!/usr/bin/env python3
"""One long gzip member written in PARTS (flate_hip_one_writer_*) against the whole call
(flate_hip_deflate_fast_spliced_framed).

    python tools/one_writer_bench.py [--mib 1024] [--reps 5] [--parts 16,64,256,1024] [--piece 65535]

The input is --mib MiB of S-text resident on the device, written as ONE gzip member in pieces of --piece bytes.  A PASS
writes the whole input through the writer in parts of P MiB of input (a part begins where the last call's in_used ends:
a slice of the resident input, nothing is moved) into one output buffer, with device pointers.  Per P: best of --reps
passes, each ALTERNATED in this process with one whole call; calls per pass, the time per call (pass / calls, and the
fastest and the median single call of the best pass).  The first pass of every P is held, call by call, against the
whole call's bytes.  One pass with host pointers and 64 MiB parts, and flate_hip_stream_write on the first 8 MiB for the
ratio to the piecewise writer that was there before.  `spread` is the largest difference between two runs of the same
kind (the first, which sizes the scratch, left out).  Prints one JSON line; also written to $FLATE_OUT_ROOT (default
results/)/one_writer_bench.json."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
flate = importlib.import_module("moonbit-flate_amd")
MIB = 1 << 20
WINDOW = 65535


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", default="16,64,256,1024")
    ap.add_argument("--piece", type=int, default=65535)
    a = ap.parse_args()
    import torch

    t0 = time.perf_counter()
    h = flate.synth("text", a.mib * 16, 65536)
    T, P = int(h.size), a.piece
    print("%d bytes ready in %.1f s" % (T, time.perf_counter() - t0), file=sys.stderr, flush=True)
    d = torch.from_numpy(h).cuda()
    eng = flate.FlateEngine(0)
    in_off = np.array(list(range(0, T, P)) + [T], dtype=np.uint64)
    room = T // 2 + T // 8 + (1 << 20)  # (S-text compresses to under a half; a call that does not fit fails the run)
    whole_out = torch.empty(room, dtype=torch.uint8, device="cuda")
    res = {"what": "S-text as one gzip member, whole passes, ms", "plain_bytes": T, "piece_bytes": P, "reps": a.reps,
           "build_id": flate.build_id()}

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, round((time.perf_counter() - t) * 1e3, 3)

    def whole():
        _, n, _ = eng.deflate_spliced_framed(d, in_off, "gzip", out=whole_out, out_cap=room, index=True)
        return n

    def spread(t):
        return round(max(t[1:]) - min(t[1:]), 3)

    member_bytes = whole()
    res["member_bytes"] = member_bytes

    def a_pass(data, part, out, check):
        """The whole input through the writer -> (calls, the single calls' ms)."""
        wr = eng.open_one_writer("gzip", P, device=flate.engine._is_torch(data))
        pos, total, each = 0, 0, []
        while True:
            end = min(pos + part, T)
            t = time.perf_counter()
            used, got, r = wr.write(data[pos:end], final=end == T, out=out)
            each.append(round((time.perf_counter() - t) * 1e3, 3))
            assert r.rc in (0, 1) and (used or r.rc == 1), (r, pos)
            if check:
                assert bool((got == whole_out[total:total + r.out_len]).all()), pos
            total += r.out_len
            pos += used
            if r.rc == 1:
                break
        wr.close()
        assert total == member_bytes and pos == T, (total, pos)
        return len(each), each

    for p in [int(x) for x in a.parts.split(",")]:
        part = min(p * MIB, T)
        out = torch.empty(part // 2 + part // 8 + (1 << 20), dtype=torch.uint8, device="cuda")
        tp, tw, best_each = [], [], None
        for rep in range(a.reps + 1):  # (the first pair sizes the scratch)
            (calls, each), t = timed(lambda: a_pass(d, part, out, rep == 0))
            if rep and t <= min(tp[1:] + [t]):
                best_each = each
            tp.append(t)
            tw.append(timed(whole)[1])
        full = sorted(best_each[:-1] or best_each)  # (the last call is the shorter one)
        res["parts_%d_mib" % p] = {"pass_ms_best": min(tp[1:]), "pass_ms_all": tp, "pass_spread_ms": spread(tp),
                                   "whole_ms_best": min(tw[1:]), "whole_ms_all": tw, "whole_spread_ms": spread(tw),
                                   "calls": calls, "ms_per_call": round(min(tp[1:]) / calls, 3),
                                   "call_ms_min": full[0], "call_ms_median": full[len(full) // 2],
                                   "in_gib_per_s": round(T / 2.0**30 / (min(tp[1:]) / 1e3), 2)}
        print(json.dumps({p: res["parts_%d_mib" % p]}), file=sys.stderr, flush=True)
        del out
    part = min(64 * MIB, T)
    out = np.zeros(part // 2 + part // 8 + (1 << 20), np.uint8)
    (calls, each), t = timed(lambda: a_pass(h, part, out, False))
    res["host_pointers_64_mib"] = {"pass_ms": t, "calls": calls, "in_gib_per_s": round(T / 2.0**30 / (t / 1e3), 2)}
    n = min(8 * MIB, T) // WINDOW * WINDOW
    sw = flate.StreamWriter(eng)
    piece = h[:n]

    def old():
        return len(sw.write(piece)) + len(sw.close())
    got, t = timed(old)
    res["stream_write_8_mib"] = {"ms": t, "in_bytes": n, "out_bytes": got, "in_mb_per_s": round(n / 1e6 / (t / 1e3), 2)}
    eng.close()
    line = json.dumps(res)
    print(line)
    out_root = os.environ.get("FLATE_OUT_ROOT", os.path.join(ROOT, "results"))
    os.makedirs(out_root, exist_ok=True)
    with open(os.path.join(out_root, "one_writer_bench.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
