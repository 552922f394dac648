#!/usr/bin/env python3
"""A BGZF file read and written in PARTS (flate_hip_bgzf_reader_* / flate_hip_bgzf_writer_*) against the calls a caller
has without them.

    python tools/bgzf_parts_bench.py [--mib 1024] [--reps 5] [--parts 16,64,256] [--whole-only] [--limit 120]

The input is --mib MiB of S-text; the file is what flate_hip_bgzf_write makes of it at the default block size (1 GiB:
16 450 members, the README BGZF row's file), resident on the device; device pointers, whole passes.
  reader  the whole file through the reader in parts of P MiB of compressed bytes (a part begins where the last call's
          in_used ends: a slice of the resident file, nothing is moved) into one output buffer of 4 P MiB; against
          flate_hip_bgzf_read whole, and at P = 64 against flate_hip_gzfile_reader_read with serial_max = 1 MiB and the
          same parts -- what a caller who streams a BGZF file has today
  writer  the whole input through the writer in parts of P MiB; against flate_hip_bgzf_write whole
Per P: best of --reps passes behind one that sizes the scratch, each ALTERNATED in this process with its comparison on
the same card; `spread` is the largest difference between two passes of the same kind.  per_call_ms = (parts - whole) /
calls.  --whole-only: flate_hip_bgzf_read, flate_hip_bgzf_index and flate_hip_bgzf_write alone, --reps + 1 times each
(for a comparison between two builds of the library, FLATE_HIP_LIB).  Every timed step runs under --limit seconds: a
step that takes longer ends the process; nothing is tried twice.  Host pointers, per-kernel times and other files are
not measured.  Prints one JSON line; also written to $FLATE_OUT_ROOT (default results/)/bgzf_parts_bench.json."""
import argparse
import importlib
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
flate = importlib.import_module("moonbit-flate_amd")
MIB = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", default="16,64,256")
    ap.add_argument("--whole-only", action="store_true")
    ap.add_argument("--limit", type=int, default=120)
    a = ap.parse_args()
    import torch

    def over(*_):
        print("a timed step ran longer than %d s" % a.limit, file=sys.stderr, flush=True)
        os._exit(3)
    signal.signal(signal.SIGALRM, over)

    plain = flate.synth("text", a.mib * 16, 65536)
    T = int(plain.size)
    eng = flate.FlateEngine(0)
    d_plain = torch.from_numpy(plain).cuda()
    file_buf, n = eng.bgzf_write(d_plain)
    n = int(n)
    d = file_buf[:n]
    whole_out = torch.empty(T + 16, dtype=torch.uint8, device="cuda")
    whole_file = torch.empty(flate.engine.bgzf_bound(T), dtype=torch.uint8, device="cuda")
    res = {"what": "a BGZF file of S-text at the default block size, whole passes, ms, device pointers", "plain_bytes": T,
           "file_bytes": n, "reps": a.reps, "build_id": flate.build_id(),
           "not_measured": ["host pointers", "per-kernel times", "other files"]}

    def timed(fn):
        torch.cuda.synchronize()
        signal.alarm(a.limit)
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        t = round((time.perf_counter() - t) * 1e3, 3)
        signal.alarm(0)
        return r, t

    def stats(t):
        return {"ms_best": min(t[1:]) if len(t) > 1 else t[0], "ms_all": t,
                "spread_ms": round(max(t[1:]) - min(t[1:]), 3) if len(t) > 2 else 0.0}

    def whole_read():
        _, q = eng.bgzf_read(d, out=whole_out)
        assert q.rc == 0 and q.out_len == T, q
        return q

    def whole_index():
        q = eng.bgzf_index(d, query=True)
        assert q.rc == 0, q
        return q

    def whole_write():
        _, k = eng.bgzf_write(d_plain, out=whole_file)
        assert int(k) == n
        return k

    members = whole_read().n_members
    res["members"] = members
    if a.whole_only:
        tr, ti, tw = [], [], []
        for _ in range(a.reps + 1):
            tr.append(timed(whole_read)[1])
            ti.append(timed(whole_index)[1])
            tw.append(timed(whole_write)[1])
        res["bgzf_read"], res["bgzf_index"], res["bgzf_write"] = stats(tr), stats(ti), stats(tw)
    else:
        def read_pass(open_reader, part, out, check, count=True):
            rd = open_reader()
            pos, calls, total, got_members = 0, 0, 0, 0
            while True:
                end = min(pos + part, n)
                used, got, r = rd.read(d[pos:end], final=end == n, out=out)
                calls += 1
                assert r.rc in (0, 1) and (used or r.out_len), (r, pos)
                if check and calls == 2:
                    assert bool((got == whole_out[total:total + r.out_len]).all())
                total, pos, got_members = total + r.out_len, pos + used, got_members + r.n_members
                if r.rc == 1:
                    break
            rd.close()
            assert total == T and pos == n and (not count or got_members == members), (total, pos, got_members)
            return calls

        def write_pass(part, out, check):
            wr = eng.open_bgzf_writer(device=True)
            pos, calls, total = 0, 0, 0
            while True:
                end = min(pos + part, T)
                used, got, r = wr.write(d_plain[pos:end], final=end == T, out=out)
                calls += 1
                assert r.rc in (0, 1), r
                if check:
                    assert bool((got == d[total:total + r.out_len]).all())
                total, pos = total + r.out_len, pos + used
                if r.rc == 1:
                    break
            wr.close()
            assert total == n and pos == T, (total, pos)
            return calls

        for p in [int(x) for x in a.parts.split(",")]:
            part = p * MIB
            out = torch.empty(4 * part, dtype=torch.uint8, device="cuda")
            tp, tw, tg = [], [], []
            for rep in range(a.reps + 1):  # (the first round sizes the scratch)
                calls, t = timed(lambda: read_pass(lambda: eng.open_bgzf_reader(device=True), part, out, rep == 0))
                tp.append(t)
                tw.append(timed(whole_read)[1])
                if p == 64:
                    g_calls, t = timed(lambda: read_pass(lambda: eng.open_gzfile_reader(device=True, serial_max=MIB), part, out, False, False))
                    tg.append(t)
            w = res["read_parts_%d_mib" % p] = {
                "reader": stats(tp), "calls": calls, "bgzf_read": stats(tw),
                "per_call_ms": round((stats(tp)["ms_best"] - stats(tw)["ms_best"]) / calls, 4),
                "out_mb_per_s": round(T / 1e6 / (stats(tp)["ms_best"] / 1e3), 1)}
            if tg:
                w["gzfile_reader_serial_max_1_mib"], w["gzfile_reader_calls"] = stats(tg), g_calls
                margin = max(stats(tp)["spread_ms"], stats(tg)["spread_ms"])
                w["faster_than_gzfile_reader_by_more_than_the_spreads"] = stats(tp)["ms_best"] + margin < stats(tg)["ms_best"]
            print(json.dumps({"read": {p: w}}), file=sys.stderr, flush=True)
            del out
            out = torch.empty(flate.engine.bgzf_writer_bound(part), dtype=torch.uint8, device="cuda")
            tp, tw = [], []
            for rep in range(a.reps + 1):
                calls, t = timed(lambda: write_pass(part, out, rep == 0))
                tp.append(t)
                tw.append(timed(whole_write)[1])
            w = res["write_parts_%d_mib" % p] = {
                "writer": stats(tp), "calls": calls, "bgzf_write": stats(tw),
                "per_call_ms": round((stats(tp)["ms_best"] - stats(tw)["ms_best"]) / calls, 4),
                "in_mb_per_s": round(T / 1e6 / (stats(tp)["ms_best"] / 1e3), 1)}
            print(json.dumps({"write": {p: w}}), file=sys.stderr, flush=True)
            del out
    eng.close()
    line = json.dumps(res)
    print(line)
    out_root = os.environ.get("FLATE_OUT_ROOT", os.path.join(ROOT, "results"))
    os.makedirs(out_root, exist_ok=True)
    with open(os.path.join(out_root, "bgzf_parts_bench%s.json" % ("_whole" if a.whole_only else "")), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
